"""align_many for jobs of three and more sequences, without a device: the job generator of the GPU tests (many_multi_cases.py) and
the eligibility rule of the shared launches with RV_MANY_MULTI."""
import many_cases as mc
import many_multi_cases as mm
from helpers import oracle  # noqa: F401  (puts the repository root on sys.path)
from reveal_amd import many


def test_generator_is_deterministic_and_in_range():
    a, b = mm.class_jobs(10), mm.class_jobs(10)
    assert a == b and len(a) == 10 * len(mm.CLASSES)
    assert {k for _, k, _ in a} == set(mm.K_VALUES)
    for cls, k, seqs in mm.class_jobs(30):
        assert len(seqs) == k and all(len(s) >= 1 for s in seqs), cls
        assert mm.ranks(seqs) <= mm.MAX_RANKS, (cls, k, mm.ranks(seqs))
        assert many.takes_shared_launch([s.encode() for s in seqs], multi=True)
    assert mm.corner_jobs() == mm.corner_jobs()
    sizes = {name: (len(seqs), mm.ranks(seqs)) for name, seqs, _ in mm.corner_jobs()}
    assert sizes["three_single_bases"] == (3, 6) and sizes["sixteen_single_bases"] == (16, 32)
    assert sizes["ranks_2048"][1] == 2048 and sizes["ranks_2049"][1] == 2049
    assert sizes["ranks_512"][1] == 512 and sizes["ranks_513"][1] == 513
    assert sizes["k17"][0] == 17 and sizes["k16_full"] == (16, 2048)
    for name, seqs, eligible in mm.corner_jobs():
        assert many.takes_shared_launch([s.encode() for s in seqs], multi=True) == eligible, name
    assert all(3 <= len(j) <= 5 and mm.ranks(j) <= 215 for j in mm.small_jobs(60))
    assert mm.scale_jobs(50) == mm.scale_jobs(50)
    assert all(3 <= len(j) <= 5 and all(40 <= len(s) <= 300 for s in j) for j in mm.scale_jobs(200))


def test_generator_gives_jobs_with_anchors():
    """on the oracle alone, minlength 20: more than half of the jobs of every class have an anchor, except where one sample shares
    nothing with the others; anchors are on every sample of the (sub-)index, and `dropout` gives some with fewer than k members"""
    hit = {c: 0 for c in mm.CLASSES}
    cnt = {c: 0 for c in mm.CLASSES}
    fewer = 0
    for cls, k, seqs in mm.class_jobs(20):
        anchors, T = mm.oracle_job(seqs, 20)
        cnt[cls] += 1
        hit[cls] += 1 if anchors else 0
        assert T.upper() == "".join(s + "$" for s in seqs).upper().encode()
        assert all(2 <= len(pos) <= k for _, pos in anchors)
        if cls == "dropout":
            fewer += sum(1 for _, pos in anchors if len(pos) < k)
        elif cls not in mm.NO_ANCHOR_EXPECTED and anchors:
            assert any(len(pos) == k for _, pos in anchors), cls      # the first anchor of a job is on every sample
    print("jobs with anchors", hit, "dropout anchors of fewer than k members", fewer)
    for cls in mm.CLASSES:
        if cls in mm.NO_ANCHOR_EXPECTED:
            assert hit[cls] == 0, (cls, hit[cls])
        else:
            assert 2 * hit[cls] > cnt[cls], (cls, hit[cls], cnt[cls])
    assert fewer >= 1


def test_takes_shared_launch_rule_with_multi():
    t = many.takes_shared_launch
    three = [b"A" * 681, b"C" * 682, b"G" * 682]                          # 2048 ranks
    assert t(three, multi=True) and not t(three) and not t(three, multi=False)
    assert not t([b"A" * 682, b"C" * 682, b"G" * 682], multi=True)         # 2049
    assert t([b"A"] * 16, multi=True) and not t([b"A"] * 17, multi=True)
    assert t([b"A", b"C", b"G"], multi=True)
    assert not t([b"A", b"C\0", b"G"], multi=True)
    # pairs: the switch changes nothing
    for multi in (False, True):
        assert t([b"A" * 1023, b"C" * 1023], multi=multi)
        assert not t([b"A" * 1024, b"C" * 1023], multi=multi)
        assert not t([b"A", b"C\0"], multi=multi)
    assert not t([b"A"], multi=True)
    # today's answers for every job of the pair generators
    for _, pair in mc.class_jobs(3):
        seqs = [s.encode() for s in pair]
        assert t(seqs) == t(seqs, multi=False) == t(seqs, multi=True) == (len(seqs[0]) + len(seqs[1]) + 2 <= many.LEAF_RANKS)
    assert not any(t([s.encode() for s in j]) for j in mc.multi_jobs())
    assert all(t([s.encode() for s in j], multi=True) == (mm.ranks(j) <= 2048) for j in mc.multi_jobs())
