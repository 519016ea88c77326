"""RV_MANY_LARGE_MULTI without a device: the job generator of tests/test_gpu_many_large_multi.py, the sample-major layout of a round and its
coordinate maps (reveal_amd/many.py mirrors what csrc/rv_many.hip lays out), and the eligibility rule with the new keyword."""
import bisect
import inspect

import many_cases as mc
import many_large_multi_cases as lm
import many_multi_cases as mm
from helpers import oracle  # noqa: F401  (puts the repository root on sys.path)
from reveal_amd import many


def as_bytes(job):
    return [s.encode() for s in job]


def test_generator_is_deterministic_and_in_range():
    a, b = lm.class_jobs(5), lm.class_jobs(5)
    assert a == b and len(a) == 5 * len(lm.CLASSES)
    assert lm.class_jobs(2, seed=5) != lm.class_jobs(2, seed=6)
    assert {k for _, k, _ in lm.class_jobs(2)} == set(lm.K_VALUES) == {3, 4, 5, 8, 16}
    assert lm.RANKS_MIN == many.LEAF_RANKS + 1
    seen = set()
    for cls, k, seqs in lm.class_jobs(15):
        assert len(seqs) == k and all(len(s) >= 1 for s in seqs), cls
        assert lm.RANKS_MIN <= lm.ranks(seqs) <= lm.RANKS_MAX, (cls, k, lm.ranks(seqs))
        assert many.takes_shared_launch(as_bytes(seqs), large_multi=True) and not many.takes_shared_launch(as_bytes(seqs), multi=True, large=True)
        seen.add((cls, k))
    assert {c for c, _ in seen} == set(lm.CLASSES) and len(seen) == len(lm.CLASSES) * len(lm.K_VALUES)
    assert all(len(set(seqs)) == 1 for cls, _, seqs in lm.class_jobs(5) if cls == "identical")
    sized = lm.sized_jobs(10)
    assert sized == lm.sized_jobs(10) and all(2049 <= lm.ranks(j) <= 2300 for j in sized) and {len(j) for j in sized} == {3, 4, 5, 8, 16}


def test_corner_sizes():
    c = lm.corner_jobs()
    assert c == lm.corner_jobs() and len(c) == len(lm.CORNER_NAMES)
    assert tuple(lm.ranks(j) for j in c) == lm.CORNER_RANKS == (2049, 2048, 2064, 3004, 3000, 2694, 20001, 66003)
    assert [len(j) for j in c] == [3, 3, 16, 3, 3, 3, 3, 3]
    assert all(len(s) == 128 for s in c[2])
    assert 1 in [len(s) for s in c[3]]
    assert c[4] == ["A" * 1000, "A" * 999, "A" * 998] and c[5] == ["ACG" * 300, "ACG" * 299, "ACG" * 298]
    assert [len(s) for s in c[6]] == [6666] * 3 and len(set(c[6])) == 3
    assert [len(s) for s in c[7]] == [22000] * 3 and max(lm.CORNER_RANKS) > 65536
    t = many.takes_shared_launch
    assert [t(as_bytes(j), large_multi=True) for j in c] == [True, False, True, True, True, True, True, True]
    assert t(as_bytes(c[1]), multi=True, large_multi=True)              # the neighbour of 2048 ranks stays where it is today


def test_generator_gives_jobs_with_anchors():
    """on the oracle alone, minlength 20: most jobs have an anchor, and `dropout` gives anchors of fewer than k members"""
    hit = total = fewer = 0
    for cls, k, seqs in lm.class_jobs(2):
        anchors, T = lm.oracle_job(seqs, 20)
        assert T.upper() == "".join(s + "$" for s in seqs).upper().encode()
        assert all(2 <= len(pos) <= k for _, pos in anchors)
        if cls in lm.NO_ANCHOR_EXPECTED:
            continue
        total += 1
        hit += 1 if anchors else 0
        if cls == "dropout":
            fewer += sum(1 for _, pos in anchors if len(pos) < k)
    assert 2 * hit > total and fewer >= 1


def layout_jobs():
    """mixed k in one round, ascending size as the library orders them: the corner jobs of 3 and 16 sequences, class jobs of every k"""
    jobs = [as_bytes(j) for j in lm.corner_jobs()[:6] if lm.ranks(j) > 2048] + [as_bytes(seqs) for _, _, seqs in lm.class_jobs(1)]
    return sorted(jobs, key=lambda j: sum(len(s) for s in j) + len(j))


def test_sample_major_layout_holds_every_sequence_in_its_sample():
    jobs = layout_jobs()
    assert {len(j) for j in jobs} == {3, 4, 5, 8, 16}
    text, nsep, begins = many.sample_major_layout(jobs)
    assert len(text) == sum(sum(len(s) for s in j) + len(j) for j in jobs)
    assert len(nsep) == 16 and nsep == sorted(nsep) and nsep[-1] == len(text) - 1 and all(text[p] == ord("$") for p in nsep)
    for j, seqs in enumerate(jobs):
        assert len(begins[j]) == len(seqs)
        for q, s in enumerate(seqs):
            b = begins[j][q]
            assert text[b:b + len(s) + 1] == s + b"$"
            # the sample of a position by nsep (sample_of_pos: the first separator at or behind it) is the sequence number
            assert bisect.bisect_left(nsep, b) == q == bisect.bisect_left(nsep, b + len(s))
    # sample q holds the jobs that have a q-th sequence, in the round's order
    for q in range(16):
        have = [begins[j][q] for j in range(len(jobs)) if q < len(jobs[j])]
        assert have == sorted(have) and have[0] == (nsep[q - 1] + 1 if q else 0)


def test_the_coordinate_map_is_strictly_increasing_and_round_trips():
    jobs = layout_jobs()
    text, nsep, begins = many.sample_major_layout(jobs)
    for j, seqs in enumerate(jobs):
        alone = b"".join(s + b"$" for s in seqs)
        lens = [len(s) for s in seqs]
        last = -1
        for loc in range(len(alone)):
            q, p = many.to_shared_k(loc, begins[j], lens)
            assert p > last, (j, loc)                                    # strictly increasing: ties by position come out as in the job alone
            last = p
            assert text[p] == alone[loc]
            assert bisect.bisect_left(nsep, p) == q
            assert many.to_local_k(p, q, begins[j], lens) == loc
    try:
        many.to_shared_k(len(b"".join(s + b"$" for s in jobs[0])), begins[0], [len(s) for s in jobs[0]])
        assert False, "a coordinate behind the job's text"
    except many.error:
        pass


def test_takes_shared_launch_rule_with_large_multi():
    t = many.takes_shared_launch
    assert inspect.signature(t).parameters["large_multi"].default is False
    assert inspect.signature(many.align_many).parameters["large_multi"].default is None
    at, above = [b"A" * 681, b"C" * 682, b"G" * 682], [b"A" * 682, b"C" * 682, b"G" * 682]      # 2048 and 2049 ranks
    assert not t(above) and not t(above, multi=True, large=True) and t(above, large_multi=True)
    assert not t(at, large_multi=True) and t(at, multi=True) and t(at, multi=True, large_multi=True)      # RV_MANY_MULTI's class is untouched
    pair = [b"A" * 1024, b"C" * 1023]                                                           # k = 2 above 2048 ranks: RV_MANY_LARGE's
    assert not t(pair, large_multi=True) and t(pair, large=True) and t(pair, large=True, large_multi=True)
    assert t([b"A" * 1023, b"C" * 1023], large_multi=True)
    k16, k17 = [b"A" * 128] * 16, [b"A" * 128] * 17                                             # 2064 and 2193 ranks
    assert t(k16, large_multi=True) and not t(k17, large_multi=True) and not t(k17, multi=True, large=True, large_multi=True)
    cap, over = [b"A" * 10922, b"C" * 10922, b"G" * 10921], [b"A" * 10922, b"C" * 10922, b"G" * 10922]      # 32768 and 32769 ranks
    assert t(cap, large_multi=True, large_max=32768) and not t(over, large_multi=True, large_max=32768)
    assert t(over, large_multi=True) and t(over, large_multi=True, large_max=32769)
    assert not t([b"A" * 65536, b"C" * 65536, b"G"], large_multi=True)                          # above the default RV_MANY_LARGE_MAX
    assert not t(above, large_multi=True, large_max=2048)
    assert not t([b"A" * 682, b"C\0" + b"C" * 681, b"G" * 682], large_multi=True)
    # today's answers without the keyword
    for _, pair in mc.class_jobs(2):
        seqs = as_bytes(pair)
        assert t(seqs) == t(seqs, large_multi=True)
    for j in [seqs for _, _, seqs in mm.class_jobs(2)]:                                        # at most 2048 ranks
        assert t(as_bytes(j), multi=True) and t(as_bytes(j), multi=True, large_multi=True) and not t(as_bytes(j), large_multi=True)
    for j in mc.multi_jobs():                                                                   # three and five sequences on both sides of 2048 ranks
        assert t(as_bytes(j), large_multi=True) == (mm.ranks(j) > 2048) and t(as_bytes(j), multi=True, large_multi=True)
