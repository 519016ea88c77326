"""align_many without a device: the job generator of the GPU tests, the coordinate mapping of the shared layout, and the argument
checks that happen before the library is asked for a device."""
import random

import pytest

import many_cases as mc
from helpers import assemble, oracle  # noqa: F401  (puts the repository root on sys.path)
from reveal_amd import many


def test_generator_is_deterministic_and_in_range():
    a, b = mc.class_jobs(6), mc.class_jobs(6)
    assert a == b and len(a) == 6 * len(mc.CLASSES)
    for cls, (x, y) in mc.class_jobs(36):
        assert len(x) >= 1 and len(y) >= 1
        assert len(x) + len(y) + 2 <= many.LEAF_RANKS, cls
    assert all(len(x) + len(y) + 2 > many.LEAF_RANKS for x, y in mc.big_pairs(20))
    assert sorted(len(j) for j in mc.multi_jobs()) == [3, 3, 3, 5, 5]


def test_generator_gives_jobs_with_anchors():
    """on the oracle alone: more than half of the jobs of every class have at least one anchor at minlength 20, except where
    there is nothing to anchor (unrelated sequences, length-1 sequences)"""
    hit = {c: 0 for c in mc.CLASSES}
    cnt = {c: 0 for c in mc.CLASSES}
    for cls, pair in mc.class_jobs(36):
        anchors, T = mc.oracle_job(pair, 20)
        cnt[cls] += 1
        hit[cls] += 1 if anchors else 0
        assert T.upper() == (pair[0] + "$" + pair[1] + "$").upper().encode()
    for cls in mc.CLASSES:
        if cls not in mc.NO_ANCHOR_EXPECTED:
            assert 2 * hit[cls] > cnt[cls], (cls, hit[cls], cnt[cls])
    assert sum(1 for p in mc.big_pairs(20) if mc.oracle_job(p, 20)[0]) == 20
    assert all(mc.oracle_job(j, 20)[0] for j in mc.multi_jobs())


def test_shared_layout_round_trip():
    rng = random.Random(5)
    pairs = [(mc.rnd(rng, rng.randint(1, 40)).encode(), mc.rnd(rng, rng.randint(1, 40)).encode()) for _ in range(50)]
    text, abeg, bbeg = many.shared_layout(pairs)
    assert text.count(b"$") == 100 and len(text) == sum(len(a) + len(b) + 2 for a, b in pairs)
    assert bbeg[0] == abeg[-1] + len(pairs[-1][0]) + 1               # one separator position splits the two samples of every job
    for j, (a, b) in enumerate(pairs):
        alone = a + b"$" + b + b"$"
        la = len(a)
        for loc in range(len(alone)):
            side, p = many.to_shared(loc, abeg[j], bbeg[j], la)
            assert text[p] == alone[loc]
            assert (side == 0) == (p < bbeg[0])
            assert many.to_local(p, side, abeg[j], bbeg[j], la) == loc


def test_takes_shared_launch_rule():
    assert many.takes_shared_launch([b"A" * 1023, b"C" * 1023])          # 2048 ranks
    assert not many.takes_shared_launch([b"A" * 1024, b"C" * 1023])
    assert not many.takes_shared_launch([b"A", b"C", b"G"])


@pytest.mark.parametrize("jobs", [[["ACGT"]], [["ACGT", ""]], [[("x", "ACGT"), ("y", b"")]], [[]], ["ACGT"], [[1, 2]], "ACGT"])
def test_bad_jobs_raise_before_any_device(jobs):
    with pytest.raises(many.error):
        many.align_many(jobs)


def test_bad_parameters_raise_before_any_device():
    with pytest.raises(many.error):
        many.align_many([["ACGT", "ACGT"]], minn=1)
    with pytest.raises(many.error):
        many.align_many([["ACGT", "ACGT"]], minlength=-1)


def test_job_sequences_forms():
    assert many.job_sequences([("a", "acgt"), ("b", b"ACg")]) == [b"ACGT", b"ACG"]
    assert many.job_sequences(["acgt", "ACg"], toupper=False) == [b"acgt", b"ACg"]
