"""align_many with the reference's default picker for jobs of 17 .. 64 sequences above 2048 ranks (RV_MANY_CHAIN_WIDE_LARGE), without a device: the job
list of the GPU tests and its golden file (tests/golden/many_chain_wide_large.json: `rem.align` on the reference's own index,
tools/gen_many_chain_wide_large_golden.py), the conditions that make the file a test of the picker, the admission rule of the shared launches, and the
prototype of the kernel's 64-lane arithmetic (tools/chain_multi_proto.py --cases wide_large) against the file."""
import os
import sys

import pytest

import many_cases as mc
import many_chain_wide_large_cases as cw
import many_multi_cases as mm
import many_wide_cases as mw
from helpers import oracle  # noqa: F401  (puts the repository root on sys.path)
from reveal_amd import many, schemes

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))

ON = dict(chain_wide_large=True)
OTHERS = dict(chain=True, chain_multi=True, chain_wide=True, chain_large=True, chain_large_multi=True, large=True, large_multi=True, multi=True, wide=True)


def as_bytes(fam):
    return [s.upper().encode() for s in fam]


@pytest.fixture(scope="module")
def jobs():
    return cw.jobs()


@pytest.fixture(scope="module")
def golden():
    return cw.load_golden()


def test_cases_are_deterministic_and_within_their_ranges(jobs):
    assert jobs == cw.jobs()
    assert len(jobs) == cw.N_SHUFFLED + cw.N_TIED + cw.N_SUBSET + 3 * cw.N_WIDE + 3
    assert cw.K_VALUES == (17, 32, 33, 48, 64)
    assert [n for n, _ in cw.SETS] == ["default", "wpen4", "wscore3", "star-avg", "star-med", "minl10", "wpen0"]
    for _, kw in cw.SETS + (cw.BIG_SET,):
        assert 0 <= kw.get("wpen", 1) <= many.CHAIN_WIDE_LARGE_WMAX and 0 <= kw.get("wscore", 1) <= many.CHAIN_WIDE_LARGE_WMAX
    for cls, fam in jobs:
        r = mm.ranks(fam)
        assert 17 <= len(fam) <= 64 and many.LEAF_RANKS < r
        if cls in ("shuffled", "tied", "subset"):
            assert cw.RANKS[0] <= r <= cw.RANKS[1]
        elif cls.startswith("wide:"):
            assert mw.LARGE_RANKS[0] <= r <= mw.LARGE_RANKS[1]
    for cls in ("shuffled", "tied"):
        assert {len(f) for c, f in jobs if c == cls} == set(cw.K_VALUES)
    assert [len(f) for c, f in jobs if c == "subset"] == list(cw.K_VALUES)
    assert sorted({len(f) for c, f in jobs if c.startswith("wide:")}) == [17, 33, 64]
    assert [(c, len(f), mm.ranks(f)) for c, f in jobs[-3:]] == [("corner:k17_2049", 17, 2049), ("corner:k64_2112", 64, 2112), ("corner:one_base", 20, 2871)]
    assert {len(s) for s in jobs[-2][1]} == {32} and min(len(s) for s in jobs[-1][1]) == 1
    big = cw.big_job()
    assert len(big) == 17 and len(big[0]) == 70000 and mm.ranks(big) == 118517 <= many.CHAIN_LARGE_RANKS and cw.BIG_FROM >= 1 << 16
    assert big[0][cw.BIG_FROM:cw.BIG_FROM + 1000] == big[16][:1000]      # the last piece lies where positions need 17 bits
    fill = cw.fillers(many.CHAIN_WIDE_LARGE_MIN - 1)
    assert len(fill) == many.CHAIN_WIDE_LARGE_MIN - 1 >= 1 and cw.fillers(len(fill) + 2)[:len(fill)] == fill
    assert all(len(f) == 17 and mm.ranks(f) == 2142 for f in fill)
    # every job is admitted under every set, and only with the switch
    for name, kw in cw.SETS:
        args = cw.picker_args(kw)
        for cls, fam in jobs:
            assert many.takes_shared_launch(as_bytes(fam), picker=args, minlength=kw["minlength"], **ON), (name, cls)
            assert not many.takes_shared_launch(as_bytes(fam), picker=args, minlength=kw["minlength"], **OTHERS), (name, cls)
    # rem.align's defaults do not admit the big job (--maxmums could bite, a seed could arise); its own set does
    assert not many.takes_shared_launch(as_bytes(big), picker=cw.picker_args(dict(minlength=20)), **ON)
    assert many.takes_shared_launch(as_bytes(big), picker=cw.picker_args(cw.BIG_SET[1]), **ON)
    for f in fill:
        assert many.takes_shared_launch(as_bytes(f), picker=cw.picker_args(cw.BIG_SET[1]), **ON)


def test_golden_file_is_self_consistent(jobs, golden):
    """the anchors of a job lie inside its sequences, one member per sequence at most, equal text under every member, disjoint on every sequence, and
    the upper-cased text lower-cased over them is the recorded final text"""
    assert os.path.getsize(cw.GOLDEN) < 300 * 1000
    todo = [(name, fam, golden[name][j]) for name, _ in cw.SETS for j, (_, fam) in enumerate(jobs)] + [("big", cw.big_job(), golden["big"][0])]
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
        assert cw.sha(bytes(text)) == sha, name
    assert len(golden["roots"]) == len(jobs) == len(golden["below"])
    for j, (cand, ns, members, seg) in enumerate(golden["roots"]):
        assert ns == len(jobs[j][1]) and (members == 0 or any(len(p) == members for _, p in golden["default"][j][0]))
        assert (members == 0) == (not golden["default"][j][0]) and (cand > 0 or members == 0)
    # the big job: anchors inside the first sequence at positions that need 17 bits
    assert any(1 << 16 <= p < 70000 for _, pos in golden["big"][0][0] for p in pos)


def test_the_fixture_tests_the_picker(jobs, golden):
    """conditions (a) - (g) of tools/gen_many_chain_wide_large_golden.py, the built-in picker's anchors from the CPU oracle"""
    import gen_many_chain_wide_large_golden as gen
    names = [n for n, _ in cw.SETS]
    bad = gen.conditions(cw, jobs, [r[0] for r in golden["default"]], {n: [cw.digest(r[0]) for r in golden[n]] for n in names[1:]}, golden["roots"],
                         golden["below"], golden["big_most"], lambda j: gen.builtin_anchors(cw, jobs[j][1]))
    assert not bad, bad
    # (a) - (g) spelled out
    sel = [j for j, (c, _) in enumerate(jobs) if c in ("shuffled", "tied", "subset")]
    differ = sum(gen.builtin_anchors(cw, jobs[j][1]) != sorted((l, tuple(sorted(p))) for l, p in golden["default"][j][0]) for j in sel)
    assert 3 * differ >= len(sel)
    assert sum(0 < r[2] < len(jobs[j][1]) for j, r in enumerate(golden["roots"])) >= 5
    for name in cw.WEIGHT_SETS:
        changed = [j for j in range(len(jobs)) if golden[name][j] != golden["default"][j]]
        assert len(changed) >= 5 and any(len(jobs[j][1]) > 32 for j in changed), name
    most = [max(r[0], b) for r, b in zip(golden["roots"], golden["below"])]
    assert any(r[0] > 64 for r in golden["roots"]) and min(most) <= 8
    assert sum(bool(r[3]) for r in golden["roots"]) >= 3
    assert max(most) <= cw.CAP == 256 and golden["big_most"] <= cw.CAP
    # what RV_PICK_MCHAIN_CAP = 8 has to flag: some jobs, not all
    assert 0 < sum(m > 8 for m in most) < len(jobs)


def test_what_the_shared_launches_take_under_the_switch():
    """both sides of every bound of the RV_MANY_CHAIN_WIDE_LARGE row of csrc/rv_many.hip many_classes"""
    rng = __import__("random").Random(7)
    a = mc.rnd(rng, 130)
    fam = [mc.mutate(rng, a, 0.01).encode() for _ in range(17)]                                          # 17 x 131 = 2227 ranks
    assert sum(map(len, fam)) + 17 == 2227
    args = schemes.PickerArgs(maxmums=10000)
    assert many.takes_shared_launch(fam, picker=args, **ON)
    assert not many.takes_shared_launch(fam, picker=args, **OTHERS)                                      # ... and with no other switch
    assert not many.takes_shared_launch(fam, picker=args)
    # k: 16 | 17 and 64 | 65
    assert not many.takes_shared_launch(fam[:16] + [fam[0]], picker=args, chain_large_multi=True)       # k = 17 is not RV_MANY_CHAIN_LARGE_MULTI's
    assert not many.takes_shared_launch(fam[:16], picker=args, **ON)                                     # k = 16 (2096 ranks): RV_MANY_CHAIN_LARGE_MULTI's
    assert many.takes_shared_launch(fam[:16], picker=args, chain_large_multi=True)
    piece = fam[0][:40]
    assert many.takes_shared_launch([piece] * 64, picker=args, **ON)                                     # k = 64, 2624 ranks
    assert not many.takes_shared_launch([piece] * 65, picker=args, **ON, **OTHERS)                      # k = 65: always ordinary
    # ranks: 2048 | 2049
    f2048 = [s[:120] for s in fam[:16]] + [fam[16][:111]]
    f2049 = [s[:120] for s in fam[:16]] + [fam[16][:112]]
    assert sum(map(len, f2048)) + 17 == 2048 and sum(map(len, f2049)) + 17 == 2049
    assert not many.takes_shared_launch(f2048, picker=args, **ON)                                        # 2048 ranks: RV_MANY_CHAIN_WIDE's
    assert many.takes_shared_launch(f2048, picker=args, chain_wide=True)
    assert many.takes_shared_launch(f2049, picker=args, **ON)
    assert not many.takes_shared_launch(f2049, picker=args, chain_wide=True)
    # ranks: 2^17 | 2^17 + 1
    big = mc.rnd(rng, 8000).encode()
    wide = schemes.PickerArgs(maxmums=1 << 20, seedsize=1 << 20)
    each = ((1 << 17) - 17) // 17
    top = [big[:each]] * 16 + [big[:(1 << 17) - 17 - 16 * each]]
    assert sum(map(len, top)) + 17 == 1 << 17
    assert many.takes_shared_launch(top, picker=wide, **ON)                                              # 2^17 ranks
    assert not many.takes_shared_launch([top[0] + b"A"] + top[1:], picker=wide, **ON)                    # 2^17 + 1
    assert not many.takes_shared_launch([top[0] + b"A"] + top[1:], picker=wide, large_max=1 << 20, **ON)      # ... whatever RV_MANY_LARGE_MAX says
    assert not many.takes_shared_launch(fam, picker=args, large_max=2226, **ON)                          # ... which still bounds the class
    assert many.takes_shared_launch(fam, picker=args, large_max=2227, **ON)
    # weights: 128 | 129
    W = many.CHAIN_WIDE_LARGE_WMAX
    assert W == 128
    assert many.takes_shared_launch(fam, picker=schemes.PickerArgs(maxmums=10000, wpen=W, wscore=W), **ON)
    assert not many.takes_shared_launch(fam, picker=schemes.PickerArgs(maxmums=10000, wpen=W + 1), **ON)
    assert not many.takes_shared_launch(fam, picker=schemes.PickerArgs(maxmums=10000, wscore=W + 1), **ON)
    assert many.takes_shared_launch(fam[:16], picker=schemes.PickerArgs(maxmums=10000, wscore=W + 1), chain_large_multi=True)      # (the class of 16 keeps its own bound)
    assert not many.takes_shared_launch(fam, picker=schemes.PickerArgs(maxmums=10000, wpen=-1), **ON)
    # trim off, minlength 0, a seedsize that bites, a maxmums below the job's ranks
    assert not many.takes_shared_launch(fam, picker=schemes.PickerArgs(maxmums=10000, trim=False), **ON)
    assert not many.takes_shared_launch(fam, picker=args, minlength=0, **ON)
    assert many.takes_shared_launch(fam, picker=args, minlength=1, **ON)
    assert not many.takes_shared_launch(fam, picker=schemes.PickerArgs(maxmums=10000, seedsize=130), **ON)          # a seed could arise
    assert many.takes_shared_launch(fam, picker=schemes.PickerArgs(maxmums=10000, seedsize=131), **ON)
    assert not many.takes_shared_launch(fam, picker=schemes.PickerArgs(maxmums=2226), **ON)
    assert many.takes_shared_launch(fam, picker=schemes.PickerArgs(maxmums=2227), **ON)
    assert many.takes_shared_launch(fam, picker=schemes.PickerArgs(maxmums=0), **ON)
    assert not many.takes_shared_launch([fam[0][:60] + b"\0" + fam[0][61:]] + fam[1:], picker=args, **ON)
    # no picker: the switch means nothing
    assert not many.takes_shared_launch(fam, **ON) and many.takes_shared_launch(fam, wide=True, **ON)


def test_the_keyword_and_the_environment_reach_the_library(monkeypatch):
    """align_many(.., chain_wide_large=) sets RV_MANY_CHAIN_WIDE_LARGE on the batch (no device: the batch is a stand-in), and Batch's list of
    environment variables names the switch and its threshold"""
    import inspect
    src = inspect.getsource(many.Batch.__init__)
    assert '"RV_MANY_CHAIN_WIDE_LARGE"' in src and '"RV_MANY_CHAIN_WIDE_LARGE_MIN"' in src
    seen = []

    class Stop(Exception):
        pass

    class FakeBatch:
        def __init__(self, *a, **k):
            pass

        def option(self, name, value):
            seen.append((name, value))
            if name == "RV_MANY_CHAIN_WIDE_LARGE":
                raise Stop()

        def set_picker(self, *a, **k):
            pass
    monkeypatch.setattr(many, "Batch", FakeBatch)
    with pytest.raises(Stop):
        many.align_many([["ACGT" * 40] * 17], picker=schemes.PickerArgs(), chain_wide_large=True)
    assert ("RV_MANY_CHAIN_WIDE_LARGE", 1) in seen


def test_the_prototype_reproduces_the_fixture(jobs, golden):
    """tools/chain_multi_proto.py --cases wide_large on a subsample: the 64-lane arithmetic of the kernel, restated on the reference's index module
    (the product's own index needs a device), gives the fixture's results without ever giving up -- one job of every family and k
    under the sets whose gap models differ, and the job whose positions need 17 bits"""
    import chain_multi_proto as proto
    import pin_oracle as P
    refmod = P.load_refmod(False)
    if refmod is None:
        pytest.skip("oracle/_ref/reveallib.so not built (make -C oracle refmod needs the reference's sources)")
    which = list(range(0, 5)) + list(range(cw.N_SHUFFLED, cw.N_SHUFFLED + 5)) + list(range(cw.N_SHUFFLED + cw.N_TIED, len(jobs)))
    assert {len(jobs[j][1]) for j in which} >= set(cw.K_VALUES)
    bad, gave_up = proto.run_wide_large(refmod, sets=("default", "star-avg", "star-med", "wpen0"), which=which, big=True)
    assert not bad and not gave_up, (bad, gave_up)


def test_the_golden_file_regenerates(jobs, golden):
    import pin_oracle as P
    refmod = P.load_refmod(False)
    if refmod is None:
        pytest.skip("oracle/_ref/reveallib.so not built (make -C oracle refmod needs the reference's sources)")
    for name, kw in cw.SETS:
        for j, (cls, fam) in enumerate(jobs):
            an, T, calls = cw.rem_align_recorded(fam, indexmod=refmod, **kw)
            assert (an, cw.sha(T)) == golden[name][j], (name, j, cls)
            if name == "default":
                assert tuple(int(x) for x in (calls[0] if calls else (0, len(fam), 0, 0))) == golden["roots"][j] and max([c[0] for c in calls[1:]] or [0]) == golden["below"][j], (j, cls)
    an, T, calls = cw.rem_align_recorded(cw.big_job(), indexmod=refmod, **cw.BIG_SET[1])
    assert (an, cw.sha(T)) == golden["big"][0] and max(c[0] for c in calls) == golden["big_most"]
