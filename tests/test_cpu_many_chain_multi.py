"""align_many with the reference's default picker on jobs of three and more sequences, without a device: the job list of the GPU tests and its golden
file (tests/golden/many_chain_multi.json: `rem.align` on the reference's own index, tools/gen_many_chain_multi_golden.py), the conditions that make the
fixture a test, the kernel's scan order restated on the CPU against the oracle, the admission rule of the shared launch, and the argument errors that
come before the library is asked for a device."""
import json
import os
import sys

import pytest

import many_chain_multi_cases as cm
import many_multi_cases as mm
from helpers import assemble, oracle
from reveal_amd import many, schemes

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))


def as_bytes(job):
    return [s.upper().encode() for s in job]


@pytest.fixture(scope="module")
def jobs():
    return cm.jobs()


@pytest.fixture(scope="module")
def golden():
    return cm.load_golden()


def test_cases_are_deterministic_and_admitted(jobs):
    assert jobs == cm.jobs()
    assert len(jobs) == 9 * cm.PER_CLASS + cm.N_REARRANGED + len(cm.CORNERS) + 8
    assert [(c, len(f)) for c, f in jobs[:9 * cm.PER_CLASS]] == [(c, k) for c, k, _ in mm.class_jobs(cm.PER_CLASS)]
    assert sum(f == g for (c, f), (_, _, g) in zip(jobs, mm.class_jobs(cm.PER_CLASS))) >= 9 * cm.PER_CLASS - 2      # (all but the ones cut to 2048 ranks)
    assert sorted({len(f) for c, f in jobs if c == "rearranged"}) == [3, 4, 5, 8, 16]
    by = dict(jobs)
    assert [mm.ranks(by["corner:" + n]) for n in cm.CORNERS] == [6, 32, 512, 513, 2048, 2048] and len(by["corner:k16_full"]) == 16
    assert [n for n, _ in cm.SETS] == ["default", "wpen4", "wscore3", "star-avg", "star-med", "minl10", "minl1", "minn3"]
    for name, kw in cm.SETS:
        args = cm.picker_args(kw)
        for cls, fam in jobs:
            assert 3 <= len(fam) <= 16 and mm.ranks(fam) <= 2048
            assert many.takes_shared_launch(as_bytes(fam), picker=args, chain_multi=True, minlength=kw["minlength"]), (name, cls)
            # the other switches mean nothing for such a job under a picker
            assert not many.takes_shared_launch(as_bytes(fam), picker=args, chain=True, multi=True, large=True, large_multi=True, wide=True, minlength=kw["minlength"])


def test_fixture_conditions_hold_in_the_file(jobs):
    """(a) nothing raised in the reference, (b) half of the jobs reach `segment` or anchor a proper sample subset, (c) half differ from the built-in
    picker, (d) every other set changes at least 10 jobs -- checked by the generator's own function on the file as committed"""
    import gen_many_chain_multi_golden as gen
    with open(cm.GOLDEN) as f:
        doc = json.load(f)
    assert os.path.getsize(cm.GOLDEN) < 256 * 1024
    lines = gen.fixture_conditions(cm, jobs, doc)
    print("\n".join(lines))
    assert len(lines) == 2 + len(cm.SETS) - 1


def test_golden_file_is_self_consistent(jobs, golden):
    """members of an anchor lie inside their sequences, one per sample, with equal text under them; the anchors of a job cover disjoint text; the
    upper-cased text lower-cased over them is the recorded final text"""
    for name, kw in cm.SETS:
        assert len(golden[name]) == len(jobs)
        for (cls, fam), (anchors, sha) in zip(jobs, golden[name]):
            text = bytearray(("$".join(s.upper() for s in fam) + "$").encode())
            assert anchors == sorted(anchors)
            covered = bytearray(len(text))
            for (l, pos), smp in zip(anchors, cm.sample_sets(fam, anchors)):
                assert l >= kw["minlength"] and kw.get("minn", 2) <= len(pos) == len(smp) <= len(fam), (name, cls)
                for p in pos:
                    assert b"$" not in text[p:p + l] and text[p:p + l].upper() == text[pos[0]:pos[0] + l].upper() and not any(covered[p:p + l]), (name, cls)
                    covered[p:p + l] = b"\1" * l
                    text[p:p + l] = text[p:p + l].lower()
            assert cm.sha(bytes(text)) == sha, (name, cls)


def test_constructed_jobs_do_what_they_were_made_for(jobs, golden):
    by = {c: golden["default"][j][0] for j, (c, f) in enumerate(jobs)}
    fam = dict(jobs)
    sets = lambda c: cm.sample_sets(fam[c], by[c])
    # the `rest` child of two samples anchors itself
    assert frozenset((0, 1)) in sets("made:two_pairs") and frozenset((2, 3)) in sets("made:two_pairs")
    # equal z: the group `segment` saw first goes first, the other anchors in the rest child
    assert sorted(sets("made:two_pairs_tie"), key=sorted) == [frozenset((0, 1)), frozenset((2, 3))]
    assert sorted(sets("made:two_pairs_tie_interleaved"), key=sorted) == [frozenset((0, 2)), frozenset((1, 3))]
    assert frozenset((0, 1, 3, 4)) in sets("made:five_one_unrelated")
    assert frozenset((0, 1, 2)) in sets("made:down_to_two") and frozenset((0, 1)) in sets("made:down_to_two")
    for c in ("made:tandem3", "made:tandem4", "made:tandem_mixed"):
        assert len(by[c]) >= 2


def test_the_kernels_scan_lists_what_the_oracle_lists_in_its_order(jobs):
    """k_leaf_multi_chain's scan (a lane per upper rank, windows by growing size) restated in many_chain_multi_cases.kernel_scan against
    ro_getmultimums on the root index: the same matches, members in rank order, in the order `segment` breaks its tie by"""
    O = oracle(False)
    some = 0
    for cls, fam in jobs[::2]:
        T, nsep, nodes = assemble(list(fam), toupper=False)
        c = O.construct(T, nsep, len(fam))
        for minl, minn in ((1, 2), (20, 2), (10, 3)):
            l, n, off, so, pos = O.getmultimums(c["tbuf"], c["SA"], c["LCP"], c["SO"], c["nsep"], len(fam), minl=minl, minn=minn)
            want = [(int(l[k]), tuple(int(x) for x in pos[off[k]:off[k + 1]])) for k in range(len(l))]
            assert cm.kernel_scan(T, c["SA"], c["LCP"], len(fam), minl, minn) == want, (cls, minl, minn)
            some += len(want) > 1
    assert some > 50


def test_what_the_shared_launch_does_not_take():
    rng = __import__("random").Random(5)
    fam = as_bytes(mm.sized_job(rng, 3, 2048))
    small = as_bytes(mm.sized_job(rng, 4, 404))                 # four sequences of 100 bases
    args = schemes.PickerArgs(maxmums=10000)
    T = lambda seqs, p=args, **k: many.takes_shared_launch(seqs, picker=p, chain_multi=True, **k)
    assert T(fam) and not T([fam[0] + b"A"] + fam[1:])                                           # 2048 / 2049 ranks
    assert T(small) and T(small * 4) and not T(small * 4 + [small[0]])                           # 16 / 17 sequences
    assert not many.takes_shared_launch(small, picker=args, chain=True, multi=True)              # the new switch alone decides
    assert not many.takes_shared_launch(small, picker=args, chain_multi=False)
    assert not T(small, schemes.PickerArgs(maxmums=10000, seedsize=30))                          # a seed could arise
    assert not T(small, schemes.PickerArgs(maxmums=10000, seedsize=100)) and T(small, schemes.PickerArgs(maxmums=10000, seedsize=101))
    assert T(small, schemes.PickerArgs(maxmums=10000, seedsize=0))
    assert not T(small, schemes.PickerArgs(maxmums=10000, trim=False))
    assert not T(small, schemes.PickerArgs(maxmums=403)) and T(small, schemes.PickerArgs(maxmums=404))      # the cap could bite below the job's ranks
    assert T(fam, schemes.PickerArgs(maxmums=10000))                                             # rem.align's default passes at 2048 ranks
    assert not T(small, minlength=0)                                                             # the p-value cut stays on the host
    assert not T(small, schemes.PickerArgs(maxmums=10000, wpen=-1))
    assert T(small, schemes.PickerArgs(maxmums=10000, wscore=many.CHAIN_MULTI_WMAX)) and not T(small, schemes.PickerArgs(maxmums=10000, wscore=many.CHAIN_MULTI_WMAX + 1))
    assert not T(small, schemes.PickerArgs(maxmums=10000, wpen=many.CHAIN_MULTI_WMAX + 1))
    assert not T(small[:3] + [b"AC\0GT"])
    # the pair rule is untouched by the new switch, and the existing false cases stay false without it
    pair = small[:2]
    assert many.takes_shared_launch(pair, picker=args, chain=True) and many.takes_shared_launch(pair, picker=args, chain=True, chain_multi=True)
    assert not many.takes_shared_launch(pair, picker=args, chain_multi=True)
    assert not many.takes_shared_launch(small[:3], picker=args, chain=True) and not many.takes_shared_launch(small[:3], picker=args, chain=True, chain_multi=False)
    # without a picker nothing changes
    assert many.takes_shared_launch(small, multi=True, chain_multi=True) and not many.takes_shared_launch(small, chain_multi=True)


@pytest.mark.parametrize("bad", [dict(maxdepth=3), dict(maxsize=100)])
def test_unsupported_picker_options_raise_before_any_device(bad, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the library was asked for a device")
    monkeypatch.setattr(many, "Batch", no_device)
    job = ["ACGT" * 10] * 3
    with pytest.raises(many.error, match="maxbubblesize / maxdepth"):
        many.align_many([job], picker=schemes.PickerArgs(**bad), chain_multi=True)
    with pytest.raises(many.error, match="gap cost model"):
        many.align_many([job], picker=schemes.PickerArgs(gcmodel="affine"), chain_multi=True)
    with pytest.raises(many.error, match="empty"):
        many.align_many([["ACGT", "", "ACGT"]], picker=schemes.PickerArgs(), chain_multi=True)


def test_a_sample_of_the_golden_regenerates(jobs, golden):
    import pin_oracle as P
    refmod = P.load_refmod(False)
    if refmod is None:
        pytest.skip("oracle/_ref/reveallib.so not built (make -C oracle refmod needs the reference's sources)")
    for name, kw in cm.SETS:
        for j in list(range(0, len(jobs), 7)) + list(range(len(jobs) - 14, len(jobs))):
            an, T = cm.rem_align_job(list(jobs[j][1]), indexmod=refmod, **kw)
            assert (an, cm.sha(T)) == golden[name][j], (name, j, jobs[j][0])
