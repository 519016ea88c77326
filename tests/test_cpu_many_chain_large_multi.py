"""align_many with the reference's default picker for jobs of 3 .. 16 sequences above 2048 ranks (RV_MANY_CHAIN_LARGE_MULTI), without a device: the job
list of the GPU tests and its golden file (tests/golden/many_chain_large_multi.json: `rem.align` on the reference's own index,
tools/gen_many_chain_large_multi_golden.py), the conditions that make the file a test of the picker, and the admission rule of the shared launches."""
import os
import sys

import pytest

import many_cases as mc
import many_chain_large_multi_cases as cl
import many_large_multi_cases as lm
import many_multi_cases as mm
from helpers import oracle  # noqa: F401  (puts the repository root on sys.path)
from reveal_amd import many, schemes

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))


def as_bytes(fam):
    return [s.upper().encode() for s in fam]


@pytest.fixture(scope="module")
def jobs():
    return cl.jobs()


@pytest.fixture(scope="module")
def golden():
    return cl.load_golden()


def test_cases_are_deterministic_and_within_their_ranges(jobs):
    assert jobs == cl.jobs()
    ncls = cl.PER_CLASS * len(lm.CLASSES)
    assert len(jobs) == ncls + cl.N_SHUFFLED + cl.N_TIED + cl.N_SUBSET + 3
    assert [(c, f) for c, f in jobs[:ncls]] == [(c, list(f)) for c, _, f in lm.class_jobs(cl.PER_CLASS)]
    assert [n for n, _ in cl.SETS] == ["default", "wpen4", "wscore3", "star-avg", "star-med", "minl10", "wpen0"]
    for cls, fam in jobs:
        r = mm.ranks(fam)
        assert 3 <= len(fam) <= 16
        if cls in ("shuffled", "tied", "subset"):
            assert cl.RANKS[0] <= r <= cl.RANKS[1]
        elif cls in lm.CLASSES:
            assert lm.RANKS_MIN <= r <= lm.RANKS_MAX
    assert {len(f) for c, f in jobs if c == "shuffled"} == {len(f) for c, f in jobs if c == "tied"} == set(cl.K_VALUES)
    assert [(len(f), mm.ranks(f)) for _, f in jobs[-3:]] == [(3, 2049), (16, 2064), (3, 3004)] and min(len(s) for s in jobs[-1][1]) == 1
    big = cl.big_job()
    assert mm.ranks(big) == 130003 <= many.CHAIN_LARGE_RANKS and len(big[0]) > 1 << 16      # positions inside the first sequence need 17 bits
    assert len(cl.fillers(many.CHAIN_LARGE_MULTI_MIN - 1)) == many.CHAIN_LARGE_MULTI_MIN - 1
    # every job is admitted under every set, and only with the switch
    for name, kw in cl.SETS:
        args = cl.picker_args(kw)
        for cls, fam in jobs:
            assert many.takes_shared_launch(as_bytes(fam), picker=args, chain_large_multi=True, minlength=kw["minlength"]), (name, cls)
            assert not many.takes_shared_launch(as_bytes(fam), picker=args, chain=True, chain_multi=True, chain_wide=True, chain_large=True, large=True, large_multi=True,
                                                multi=True, minlength=kw["minlength"]), (name, cls)
    # rem.align's defaults do not admit the big job (--maxmums could bite, a seed could arise); its own set does
    assert not many.takes_shared_launch(as_bytes(big), picker=cl.picker_args(dict(minlength=20)), chain_large_multi=True)
    assert many.takes_shared_launch(as_bytes(big), picker=cl.picker_args(cl.BIG_SET[1]), chain_large_multi=True)
    for f in cl.fillers(3):
        assert many.takes_shared_launch(as_bytes(f), picker=cl.picker_args(cl.BIG_SET[1]), chain_large_multi=True)


def test_golden_file_is_self_consistent(jobs, golden):
    """the anchors of a job lie inside its sequences, one member per sequence at most, equal text under every member, disjoint on every sequence, and
    the upper-cased text lower-cased over them is the recorded final text"""
    todo = [(name, fam, golden[name][j]) for name, _ in cl.SETS for j, (_, fam) in enumerate(jobs)] + [("big", cl.big_job(), golden["big"][0])]
    for name, fam, (anchors, sha) in todo:
        text = bytearray(("".join(s.upper() + "$" for s in fam)).encode())
        ends, at = [], 0
        for s in fam:
            at += len(s) + 1
            ends.append(at)
        assert anchors == sorted(anchors)
        covered = bytearray(len(text))
        for l, pos in anchors:
            smp = [next(q for q, e in enumerate(ends) if p < e) for p in pos]
            assert l >= 1 and 2 <= len(pos) <= len(fam) and len(set(smp)) == len(smp), name
            for p, q in zip(pos, smp):
                assert p + l <= ends[q] - 1 and text[p:p + l] == text[pos[0]:pos[0] + l], name
                assert not any(covered[p:p + l]), (name, "not disjoint")
                covered[p:p + l] = b"\1" * l
        for l, pos in anchors:
            for p in pos:
                text[p:p + l] = text[p:p + l].lower()
        assert cl.sha(bytes(text)) == sha, name
    assert len(golden["roots"]) == len(jobs) == len(golden["below"])
    for j, (cand, ns, members, seg) in enumerate(golden["roots"]):
        assert ns == len(jobs[j][1]) and (members == 0 or any(len(p) == members for _, p in golden["default"][j][0]))
        assert (members == 0) == (not golden["default"][j][0]) and (cand > 0 or members == 0)


def test_the_fixture_tests_the_picker(jobs, golden):
    """conditions (a) - (e) of tools/gen_many_chain_large_multi_golden.py, the built-in picker's anchors from the CPU oracle"""
    import gen_many_chain_large_multi_golden as gen
    names = [n for n, _ in cl.SETS]
    bad = gen.conditions(cl, jobs, [r[0] for r in golden["default"]], {n: [cl.digest(r[0]) for r in golden[n]] for n in names[1:]}, golden["roots"],
                         golden["below"], lambda j: gen.builtin_anchors(cl, jobs[j][1]))
    assert not bad, bad
    # (a) - (e) spelled out
    sel = [j for j, (c, _) in enumerate(jobs) if c in gen.PICKER_CLASSES]
    differ = sum(gen.builtin_anchors(cl, jobs[j][1]) != sorted((l, tuple(sorted(p))) for l, p in golden["default"][j][0]) for j in sel)
    assert 3 * differ >= len(sel)
    assert sum(0 < r[2] < len(jobs[j][1]) for j, r in enumerate(golden["roots"])) >= 5
    for name in cl.WEIGHT_SETS:
        assert sum(golden[name][j] != golden["default"][j] for j in range(len(jobs))) >= 5, name
    assert any(r[0] > 64 for r in golden["roots"]) and any(max(r[0], b) <= 8 for r, b in zip(golden["roots"], golden["below"]))
    assert sum(bool(r[3]) for r in golden["roots"]) >= 3
    # what RV_PICK_MCHAIN_CAP = 8 has to flag: some jobs, not all
    over = [max(r[0], b) > 8 for r, b in zip(golden["roots"], golden["below"])]
    assert 0 < sum(over) < len(jobs)


def test_what_the_shared_launches_take_under_the_switch():
    rng = __import__("random").Random(6)
    a = mc.rnd(rng, 700)
    fam = [a.encode(), mc.mutate(rng, a, 0.01).encode(), mc.mutate(rng, a, 0.01).encode()]            # 2103 ranks
    args = schemes.PickerArgs(maxmums=10000)
    on = dict(chain_large_multi=True)
    assert many.takes_shared_launch(fam, picker=args, **on)
    assert not many.takes_shared_launch(fam, picker=args, chain=True, chain_multi=True, chain_wide=True, chain_large=True)      # ... and not without the switch
    f2048 = [fam[0][:682], fam[1][:682], fam[2][:681]]
    f2049 = [fam[0][:682], fam[1][:682], fam[2][:682]]
    assert sum(map(len, f2048)) + 3 == 2048 and sum(map(len, f2049)) + 3 == 2049
    assert not many.takes_shared_launch(f2048, picker=args, **on)                                        # 2048 ranks: RV_MANY_CHAIN_MULTI's
    assert many.takes_shared_launch(f2048, picker=args, chain_multi=True, **on)
    assert many.takes_shared_launch(f2049, picker=args, **on)
    assert not many.takes_shared_launch(f2049, picker=args, chain_multi=True)
    piece = fam[0][:150]
    assert not many.takes_shared_launch([fam[0] + fam[1], fam[2] + fam[0]], picker=args, **on)           # k = 2: RV_MANY_CHAIN_LARGE's
    assert many.takes_shared_launch([fam[0] + fam[1], fam[2] + fam[0]], picker=args, chain_large=True, **on)
    assert many.takes_shared_launch([piece] * 16, picker=args, **on)                                     # k = 16, 2416 ranks
    assert not many.takes_shared_launch([piece] * 17, picker=args, chain_wide=True, **on)               # k = 17: ordinary under a picker above 2048 ranks
    big = mc.rnd(rng, 1 << 16).encode()
    wide = schemes.PickerArgs(maxmums=1 << 20, seedsize=1 << 20)
    third = ((1 << 17) - 3) // 3
    top = [big[:third], big[:third], big[:(1 << 17) - 3 - 2 * third]]
    assert sum(map(len, top)) + 3 == 1 << 17
    assert many.takes_shared_launch(top, picker=wide, **on)                                              # 2^17 ranks
    assert not many.takes_shared_launch([top[0] + b"A", top[1], top[2]], picker=wide, **on)              # 2^17 + 1
    assert not many.takes_shared_launch([top[0] + b"A", top[1], top[2]], picker=wide, large_max=1 << 20, **on)      # ... whatever RV_MANY_LARGE_MAX says
    assert not many.takes_shared_launch(fam, picker=args, large_max=2100, **on)                          # ... which still bounds the class
    assert not many.takes_shared_launch(fam, picker=schemes.PickerArgs(maxmums=2102), **on)              # maxmums just below the ranks
    assert many.takes_shared_launch(fam, picker=schemes.PickerArgs(maxmums=2103), **on)
    assert many.takes_shared_launch(fam, picker=schemes.PickerArgs(maxmums=0), **on)
    assert not many.takes_shared_launch(fam, picker=schemes.PickerArgs(maxmums=10000, wpen=1025), **on)             # a weight of 1025
    assert not many.takes_shared_launch(fam, picker=schemes.PickerArgs(maxmums=10000, wscore=1025), **on)
    assert not many.takes_shared_launch(fam, picker=schemes.PickerArgs(maxmums=10000, wpen=many.CHAIN_LARGE_MULTI_WMAX + 1), **on)      # the class' own bound: 512
    assert many.takes_shared_launch(fam, picker=schemes.PickerArgs(maxmums=10000, wpen=many.CHAIN_LARGE_MULTI_WMAX, wscore=many.CHAIN_LARGE_MULTI_WMAX), **on)
    assert not many.takes_shared_launch(fam, picker=schemes.PickerArgs(maxmums=10000, wpen=-1), **on)
    assert not many.takes_shared_launch(fam, picker=args, minlength=0, **on)                             # minlength 0: the p-value cut stays on the host
    assert not many.takes_shared_launch(fam, picker=schemes.PickerArgs(maxmums=10000, trim=False), **on)
    assert not many.takes_shared_launch(fam, picker=schemes.PickerArgs(maxmums=10000, seedsize=700), **on)          # a seed could arise
    assert many.takes_shared_launch(fam, picker=schemes.PickerArgs(maxmums=10000, seedsize=701), **on)
    assert not many.takes_shared_launch([fam[0], fam[1][:300] + b"\0" + fam[1][301:], fam[2]], picker=args, **on)
    # no picker: the switch means nothing
    assert not many.takes_shared_launch(fam, **on) and many.takes_shared_launch(fam, large_multi=True, **on)
    # rem.align's defaults: jobs of up to 10 000 ranks
    dflt = cl.picker_args(dict(minlength=20))
    assert many.takes_shared_launch([big[:3332], big[:3332], big[:3333]], picker=dflt, **on)             # 10 000 ranks
    assert not many.takes_shared_launch([big[:3333], big[:3333], big[:3332]], picker=dflt, **on)         # 10 001


def test_the_keyword_reaches_the_library(monkeypatch):
    """align_many(.., chain_large_multi=) sets RV_MANY_CHAIN_LARGE_MULTI on the batch (no device: the batch is a stand-in)"""
    seen = []

    class Stop(Exception):
        pass

    class FakeBatch:
        def __init__(self, *a, **k):
            pass

        def option(self, name, value):
            seen.append((name, value))
            if name == "RV_MANY_CHAIN_LARGE_MULTI":
                raise Stop()

        def set_picker(self, *a, **k):
            pass
    monkeypatch.setattr(many, "Batch", FakeBatch)
    with pytest.raises(Stop):
        many.align_many([["ACGT" * 200] * 3], picker=schemes.PickerArgs(), chain_large_multi=True)
    assert ("RV_MANY_CHAIN_LARGE_MULTI", 1) in seen


def test_the_golden_file_regenerates(jobs, golden):
    import pin_oracle as P
    refmod = P.load_refmod(False)
    if refmod is None:
        pytest.skip("oracle/_ref/reveallib.so not built (make -C oracle refmod needs the reference's sources)")
    for name, kw in cl.SETS:
        for j, (cls, fam) in enumerate(jobs):
            an, T, calls = cl.rem_align_recorded(fam, indexmod=refmod, **kw)
            assert (an, cl.sha(T)) == golden[name][j], (name, j, cls)
            if name == "default":
                assert tuple(int(x) for x in (calls[0] if calls else (0, len(fam), 0, 0))) == golden["roots"][j] and max([c[0] for c in calls[1:]] or [0]) == golden["below"][j], (j, cls)
    an, T, _ = cl.rem_align_recorded(cl.big_job(), indexmod=refmod, **cl.BIG_SET[1])
    assert (an, cl.sha(T)) == golden["big"][0]
