"""align_many with the reference's default picker on jobs of 17 .. 64 sequences, without a device: the job list of the GPU tests and its golden file
(tests/golden/many_chain_wide.json: `rem.align` on the reference's own index, tools/gen_many_chain_wide_golden.py), the conditions that make the fixture a
test, the kernel's scan order restated on the CPU against the oracle, and the admission rule of the shared launch."""
import json
import os
import random
import sys

import pytest

import many_chain_multi_cases as cm
import many_chain_wide_cases as cw
import many_multi_cases as mm
import many_wide_cases as mw
from helpers import assemble, oracle
from reveal_amd import many, schemes

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))


def as_bytes(job):
    return [s.upper().encode() for s in job]


@pytest.fixture(scope="module")
def jobs():
    return cw.jobs()


@pytest.fixture(scope="module")
def golden():
    return cw.load_golden()


def test_cases_are_deterministic_and_admitted(jobs):
    assert jobs == cw.jobs()
    nclass, nshort = len(mw.K_VALUES) * cw.PER_K, 3 * cw.SHORT_PER_K
    assert len(jobs) == nclass + nshort + len(cw.CORNERS) + cw.N_SHUFFLED + cw.N_TIED
    assert sorted({len(f) for c, f in jobs if c == "tied"}) == [17, 33, 48, 64] and cw.HASHED_SETS == ("minl1",)
    assert [(c, len(f), f) for c, f in jobs[:nclass]] == [(c, k, list(f)) for c, k, f in mw.class_jobs(cw.PER_K)]
    assert [f for _, f in jobs[nclass:nclass + nshort]] == [list(f) for f in mw.short_jobs(cw.SHORT_PER_K)]
    by = dict(jobs)
    assert [(len(by["corner:" + n]), mm.ranks(by["corner:" + n])) for n in cw.CORNERS] == [(17, 34), (64, 128), (17, 17 * 40), (64, 2048)]
    assert sorted({len(f) for c, f in jobs if c == "shuffled"}) == [17, 24, 32, 48, 64]
    assert [n for n, _ in cw.SETS] == ["default", "minl10", "minl5", "minl1", "minn3", "minn17", "wpen4", "wpen0", "wscore3", "star-avg", "star-med"]
    assert dict(cw.SETS)["wpen4"] == dict(minlength=5, wpen=4) and dict(cw.SETS)["wscore3"] == dict(minlength=5, wscore=3)
    for name, kw in cw.SETS:
        args = cw.picker_args(kw)
        assert 0 <= args.wpen <= many.CHAIN_MULTI_WMAX and 0 <= args.wscore <= many.CHAIN_MULTI_WMAX
        for cls, fam in jobs:
            assert 17 <= len(fam) <= 64 and mm.ranks(fam) <= 2048
            assert many.takes_shared_launch(as_bytes(fam), picker=args, chain_wide=True, minlength=kw["minlength"]), (name, cls)
            # the other switches mean nothing for such a job under a picker
            assert not many.takes_shared_launch(as_bytes(fam), picker=args, chain=True, chain_multi=True, multi=True, large=True, large_multi=True, wide=True,
                                                minlength=kw["minlength"])


def test_shuffled_jobs_are_what_they_say():
    """3 .. 5 blocks of distinct lengths in every member, two of them swapped in a proper subset, the job within 2048 ranks; seven-base blocks at k = 64"""
    rng = random.Random(1)
    for k in cw.SHUFFLED_K * 3:
        fam = cw.shuffled(rng, k)
        assert len(fam) == k and mm.ranks(fam) <= 2048 and len(set(fam)) > 1
        if k == 64:
            assert min(len(s) for s in fam) >= 3 * 5 and max(len(s) for s in fam) <= 31


def test_tied_jobs_are_what_they_say():
    """every member holds the same blocks, the two longest of them equally long, in one of two orders"""
    rng = random.Random(1)
    for k in cw.TIED_K * 3:
        fam = cw.tied(rng, k)
        assert len(fam) == k and mm.ranks(fam) <= 2048 and len(set(fam)) > 1


def test_the_lane_arithmetic_of_the_wide_form_is_the_gap_cost():
    """chain_multi_proto.gapcost_lanes -- the 64-sample kernel's gap cost restated lane by lane (rank by lane with ties by lane index, a lane's share of
    the pairs, wave sums) -- against the plain definition, on random gaps over random sample sets of 2 .. 64 paths: many ties, zeros, equal gaps"""
    import chain_multi_proto as P
    rng = random.Random(11)
    for trial in range(600):
        k = rng.choice((2, 3, 16, 17, 31, 32, 33, 63, 64, rng.randint(2, 64)))
        samples = sorted(rng.sample(range(64), k))
        top = rng.choice((0, 1, 3, 40, 2047))
        d = [-rng.randint(0, top) for _ in samples]
        for model in (0, 1, 2):
            assert P.gapcost_lanes(dict(zip(samples, d)), model) == P.gapcost(d, model), (samples, d, model)
    assert P.gapcost_lanes({5: -3, 9: -3, 63: -7}, 2) == 3 and P.gapcost_lanes({0: -1, 1: -2, 2: -4}, 0) == 6 and P.gapcost_lanes({0: -5, 40: -6}, 1) == 5


def test_the_job_the_kernel_flags_by_itself():
    """many_chain_wide_cases.flagged_job(): admitted, and at minlength 1 the pick stage gives up on it with flag 8 and nothing else (the prototype, on the
    reference's index where it is built, else on the product's CPU-side modules is not possible: then the test stops at the admission)"""
    import chain_multi_proto as P
    import pin_oracle
    job = cw.flagged_job()
    assert len(job) == 17 and mm.ranks(job) <= 2048
    kw = dict(minlength=1)
    assert many.takes_shared_launch(as_bytes(job), picker=cw.picker_args(kw), chain_wide=True, minlength=1)
    refmod = pin_oracle.load_refmod(False)
    if refmod is None:
        return
    orig, stat = schemes.GraphPicker.graphmumpicker, {}
    schemes.GraphPicker.graphmumpicker = P.make_picker([s.upper() for s in job], cw.picker_args(kw), stat, orig, wide=True)
    try:
        got = cw.rem_align_job(job, indexmod=refmod, **kw)
    finally:
        schemes.GraphPicker.graphmumpicker = orig
    assert stat.get(8) == 1 and 1 not in stat and 2 not in stat
    assert got == cw.rem_align_job(job, indexmod=refmod, **kw)          # (a give-up falls back to the reference's picker: the same result)


def test_fixture_conditions_hold_in_the_file(jobs):
    """(a) nothing raised in the reference, (b) half of the jobs reach `segment` or anchor a proper sample subset, (c) half differ from the built-in
    picker, (d) every weight or gap-model set changes at least 5 jobs against minl5, one of them of 33 or more sequences, (e) every k of
    many_wide_cases.K_VALUES occurs, (f) star-avg and star-med each differ from wpen0 on at least 5 jobs and from each other on at least 5, jobs of
    33 or more sequences among them -- checked by the generator's own function on the file as committed"""
    import gen_many_chain_wide_golden as gen
    with open(cw.GOLDEN) as f:
        doc = json.load(f)
    assert os.path.getsize(cw.GOLDEN) < gen.MAX_BYTES == 288 * 1024
    lines = gen.fixture_conditions(cw, jobs, doc)
    print("\n".join(lines))
    assert len(lines) == 4 + len(cw.WEIGHT_SETS) + 3
    # a file whose star-med results were star-avg's is refused, and so is one whose star sets only switched the penalty off
    with pytest.raises(AssertionError, match=r"\(f\) star-avg  differs from star-med on 0 jobs"):
        gen.fixture_conditions(cw, jobs, dict(doc, results=dict(doc["results"], **{"star-med": [dict(same_as="star-avg")] * len(jobs)})))
    with pytest.raises(AssertionError, match=r"\(f\) star-avg  differs from wpen0    on 0 jobs"):
        gen.fixture_conditions(cw, jobs, dict(doc, results=dict(doc["results"], **{"star-avg": [dict(same_as="wpen0")] * len(jobs)})))
    # the function does refuse: a file whose weight sets equal minl5 tests nothing
    broken = dict(doc, results=dict(doc["results"], wpen4=[dict(same_as="minl5")] * len(jobs)))
    with pytest.raises(AssertionError, match="wpen4"):
        gen.fixture_conditions(cw, jobs, broken)
    with pytest.raises(AssertionError, match="raise"):
        gen.fixture_conditions(cw, jobs, dict(doc, raised=dict(doc["raised"], minl1=1)))


def test_golden_file_is_self_consistent(jobs, golden):
    """members of an anchor lie inside their sequences, one per sample, with equal text under them; the anchors of a job cover disjoint text; the
    upper-cased text lower-cased over them is the recorded final text.  (minl1 is kept as hashes and has no anchors to look at.)"""
    looked = 0
    for name, kw in cw.SETS:
        assert len(golden[name]) == len(jobs)
        if name in cw.HASHED_SETS:
            assert all(sorted(r) == ["asha", "n", "sha"] for r in golden[name])
            continue
        for (cls, fam), rec in zip(jobs, golden[name]):
            anchors = [(a[0], tuple(a[1:])) for a in rec["anchors"]]
            text = bytearray(("$".join(s.upper() for s in fam) + "$").encode())
            assert anchors == sorted(anchors)
            covered = bytearray(len(text))
            for (l, pos), smp in zip(anchors, cw.sample_sets(fam, anchors)):
                # (no l >= minlength: trim shortens a match after the length cut, a tandem family at the default set has an anchor of 6 bases)
                assert l >= 1 and kw.get("minn", 2) <= len(pos) == len(smp) <= len(fam), (name, cls)
                for p in pos:
                    assert b"$" not in text[p:p + l] and text[p:p + l].upper() == text[pos[0]:pos[0] + l].upper() and not any(covered[p:p + l]), (name, cls)
                    covered[p:p + l] = b"\1" * l
                    text[p:p + l] = text[p:p + l].lower()
                looked += 1
            assert cw.sha(bytes(text)) == rec["sha"], (name, cls)
            assert cw.same(rec, anchors, rec["sha"]) and not cw.same(rec, anchors + [(1, (0, 1))], rec["sha"])
    assert looked > 3000


def test_the_kernels_scan_lists_what_the_oracle_lists_in_its_order(jobs):
    """k_leaf_multi_chain's scan (a lane per upper rank, windows by growing size up to 64 ranks) restated in many_chain_multi_cases.kernel_scan against
    ro_getmultimums on the root index of the wide jobs: the same matches, members in rank order, in the order `segment` breaks its tie by"""
    O = oracle(False)
    some = 0
    for cls, fam in jobs[::3]:
        T, nsep, nodes = assemble(list(fam), toupper=False)
        c = O.construct(T, nsep, len(fam))
        for minl, minn in ((1, 2), (5, 2), (10, 17)):
            l, n, off, so, pos = O.getmultimums(c["tbuf"], c["SA"], c["LCP"], c["SO"], c["nsep"], len(fam), minl=minl, minn=minn)
            want = [(int(l[k]), tuple(int(x) for x in pos[off[k]:off[k + 1]])) for k in range(len(l))]
            assert cm.kernel_scan(T, c["SA"], c["LCP"], len(fam), minl, minn) == want, (cls, minl, minn)
            some += len(want) > 1
    assert some > 50


def test_what_the_shared_launch_does_not_take():
    rng = random.Random(5)
    args = schemes.PickerArgs(maxmums=10000)
    T = lambda seqs, p=args, **k: many.takes_shared_launch(seqs, picker=p, chain_wide=True, **k)
    four = as_bytes(mm.sized_job(rng, 4, 404))                   # four sequences of 100 bases
    k16, k17, k64, k65 = four * 4, four * 4 + four[:1], [s[:31] for s in four * 16], [s[:30] for s in four * 16] + [four[0][:30]]
    assert not T(k16) and T(k17) and T(k64) and not T(k65)                                       # 16 / 17 / 64 / 65 sequences
    assert mm.ranks(k64) == 2048 and not T([k64[0] + b"A"] + k64[1:])                            # 2048 / 2049 ranks
    assert T(k16, chain_multi=True)                                                              # (the narrow switch takes the job of 16)
    assert not many.takes_shared_launch(k17, picker=args, chain=True, chain_multi=True, multi=True, wide=True)      # the new switch alone decides
    assert not many.takes_shared_launch(k17, picker=args, chain_wide=False)
    assert not T(k17, schemes.PickerArgs(maxmums=10000, trim=False))
    assert not T(k17, minlength=0)                                                               # the p-value cut stays on the host
    assert not T(k17, schemes.PickerArgs(maxmums=10000, seedsize=30))                            # a seed could arise
    assert not T(k17, schemes.PickerArgs(maxmums=10000, seedsize=100)) and T(k17, schemes.PickerArgs(maxmums=10000, seedsize=101))
    assert T(k17, schemes.PickerArgs(maxmums=10000, seedsize=0))
    r17 = mm.ranks(k17)
    assert not T(k17, schemes.PickerArgs(maxmums=r17 - 1)) and T(k17, schemes.PickerArgs(maxmums=r17))      # the cap could bite below the job's ranks
    assert T(k64, schemes.PickerArgs(maxmums=10000))                                             # rem.align's default passes at 2048 ranks
    W = many.CHAIN_MULTI_WMAX
    assert W == 1024                                                                             # (the bound rv_leaf_multi_chain.hip derives for both forms)
    assert T(k17, schemes.PickerArgs(maxmums=10000, wscore=W, wpen=W))
    assert not T(k17, schemes.PickerArgs(maxmums=10000, wscore=W + 1)) and not T(k17, schemes.PickerArgs(maxmums=10000, wpen=W + 1))
    assert not T(k17, schemes.PickerArgs(maxmums=10000, wpen=-1))
    assert not T(k17[:16] + [b"AC\0GT"])
    # pairs and jobs of 3 .. 16 sequences are untouched by the new switch
    assert many.takes_shared_launch(four[:2], picker=args, chain=True, chain_wide=True) and not T(four[:2]) and not T(four)
    # without a picker nothing changes
    assert many.takes_shared_launch(k17, wide=True, chain_wide=True) and not many.takes_shared_launch(k17, chain_wide=True)


def test_without_the_switch_the_answers_are_the_old_ones():
    """chain_wide false or absent: what the function returned before, on the corner jobs of many_chain_multi_cases and many_wide_cases -- restated here
    from the rules as they stood"""
    args = schemes.PickerArgs(maxmums=10000)
    corners = [(n, f) for n, f, _ in mm.corner_jobs()] + [(n, f) for n, f, _ in mw.corner_jobs()]
    assert {"k17", "k64_2049", "k65", "k16", "ranks_2049"} <= {n for n, _ in corners}
    for name, fam in corners:
        b = as_bytes(fam)
        k, r = len(b), mm.ranks(fam)
        for extra in (dict(), dict(chain_wide=False)):
            # under a picker: pairs with chain, 3 .. 16 with chain_multi, nothing wider, nothing above 2048 ranks
            assert many.takes_shared_launch(b, picker=args, chain=True, chain_multi=True, multi=True, large=True, large_multi=True, wide=True, **extra) == \
                (2 <= k <= 16 and r <= 2048), name
            assert not many.takes_shared_launch(b, picker=args, multi=True, large=True, large_multi=True, wide=True, **extra), name
            # without one: the classes of the built-in picker
            assert many.takes_shared_launch(b, multi=True, wide=True, **extra) == ((k <= 16 and r <= 2048) or (17 <= k <= 64 and r <= many.LARGE_MAX)), name
            assert many.takes_shared_launch(b, **extra) == (k == 2 and r <= 2048), name


def test_a_sample_of_the_golden_regenerates(jobs, golden):
    import pin_oracle as P
    refmod = P.load_refmod(False)
    if refmod is None:
        pytest.skip("oracle/_ref/reveallib.so not built (make -C oracle refmod needs the reference's sources)")
    for name, kw in cw.SETS:
        for j in list(range(0, len(jobs), 9)) + list(range(len(jobs) - 6, len(jobs))):
            an, T = cw.rem_align_job(list(jobs[j][1]), indexmod=refmod, **kw)
            assert cw.same(golden[name][j], an, cw.sha(T)), (name, j, jobs[j][0])
