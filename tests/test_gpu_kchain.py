"""GPU suite: `kchain.kchain_many` / `Batch.kchain` -- the collinear chain of `reveal chain` for many jobs in one call (csrc/rv_kchain.hip) -- against
tests/golden/many_kchain.json, the reference's own chain() on the CPU oracle's list of every job ALONE (tools/gen_kchain_golden.py), job by job: path,
node scores, end score; and `chain_recurse` against kchain_recurse.json."""
import json
import os

import numpy as np
import pytest

import kchain_cases as C
from helpers import GOLD
from reveal_amd import kchain as K
from reveal_amd import many

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLD, "many_kchain.json")) as f:
    MANY = json.load(f)["runs"]


def chain(jobs, p=C.P0, sa64=False, batch=None, large=None):
    return K.kchain_many([list(j) for j in jobs], p["minlength"], p["maxmums"], p["wpen"], p["wscore"], p["gcmodel"], sa64=sa64, toupper=False, batch=batch, large=large)


def check(batch, p, chains):
    gold = MANY[C.run_key(batch, p)]
    assert len(chains) == len(gold)
    for j, want in enumerate(gold):
        got = C.digest(chains[j], chains.end_score[j])
        assert got == want, (batch, p, j, chains[j][:3], want)


def same_arrays(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def n_full(seqs, minl=20):
    return sum(1 for r in C.oracle_records(tuple(seqs), minl) if r[1] == len(seqs))


@pytest.mark.parametrize("sa64", [False, True])
def test_mixed_call(sa64):
    jobs = C.mixed_jobs()
    b = many.Batch(sa64)
    for p in C.RUNS["mixed"][:2] + [C.params(minlength=1 << 20)]:      # minlength 20, 5 and above every LCP
        chains, info = chain(jobs, p, sa64, b)
        if p["minlength"] < 1 << 20:
            check("mixed", p, chains)
        assert info["jobs"] == len(jobs) and info["ordinary"] == 2 and info["shared"] == len(jobs) - 2 and info["flagged"] == 0
    first, l, score, pos, end = chains.arrays      # above every LCP: empty paths, and p1's offer to p2 as every end score
    assert not first.any() and len(l) == len(score) == len(pos) == 0 and len(end) == len(jobs)
    for j, seqs in enumerate(jobs):
        lens = [len(s) for s in seqs]
        assert end[j] == -K.gapcost(tuple([-1] * len(lens)), tuple(lens))


@pytest.mark.parametrize("p", C.RUNS["mixed"][2:], ids=lambda p: C.run_key("mixed", p))
def test_cap_gap_models_and_weights(p):
    chains, _ = chain(C.mixed_jobs(), p)
    check("mixed", p, chains)


@pytest.mark.parametrize("sa64", [False, True])
def test_cap_through_equal_lengths(sa64):
    b = many.Batch(sa64)
    for p in C.RUNS["cap"]:
        chains, _ = chain(C.cap_jobs(), p, sa64, b)
        check("cap", p, chains)


def test_both_paths_give_equal_arrays():
    jobs = C.mixed_jobs()
    b = many.Batch()
    for p in (C.P0, C.RUNS["mixed"][3]):
        dev, info = chain(jobs, p, batch=b)
        b.option("RV_MANY_KCHAIN_HOST", 1)
        host, hinfo = chain(jobs, p, batch=b)
        b.option("RV_MANY_KCHAIN_HOST", 0)
        assert same_arrays(dev.arrays, host.arrays)
        assert hinfo["shared"] == info["shared"] and hinfo["flagged"] == 0
        check("mixed", p, host)


def test_flag_path():
    """RV_KCHAIN_CAP at 4 flags exactly the jobs with more kept candidates (cap_jobs holds pairs and triples of exactly 4 and of 5 full matches); they
    come back with the same result through the host"""
    jobs = C.cap_jobs() + C.mixed_jobs()[:40]
    b = many.Batch()
    whole, info = chain(jobs, batch=b)
    assert info["flagged"] == 0
    b.option("RV_KCHAIN_CAP", 4)
    capped, cinfo = chain(jobs, batch=b)
    counts = [n_full(s) for s in jobs]
    assert counts[0] == counts[1] == 4 and counts[2] == counts[3] == 5
    shared = [many.takes_shared_scan([x.encode("latin-1") for x in s]) for s in jobs]
    assert cinfo["flagged"] == sum(1 for c, s in zip(counts, shared) if s and c > 4) >= 8
    assert same_arrays(whole.arrays, capped.arrays)
    for j in range(len(C.cap_jobs())):
        assert C.digest(capped[j], capped.end_score[j]) == MANY[C.run_key("cap", C.P0)][j]


def test_member_cap():
    """c k = 2048 stays on the device, 2052 goes to the host: large-class jobs of k = 4 with 512 and 513 full matches"""
    jobs = C.member_jobs()
    assert [n_full(s) for s in jobs] == [512, 513]
    b = many.Batch()
    b.option("RV_MANY_SCAN_LARGE_MIN", 1)
    chains, info = chain(jobs, batch=b, large=True)
    check("members", C.P0, chains)
    assert info["shared"] == 2 and info["flagged"] == 1


@pytest.mark.parametrize("sa64", [False, True])
def test_large_class(sa64):
    jobs = C.large_jobs()
    b = many.Batch(sa64)
    for p in C.RUNS["large"]:
        on, info = chain(jobs, p, sa64, b, large=True)
        assert info["shared"] == len(jobs) and info["ordinary"] == 0
        check("large", p, on)
        off, oinfo = chain(jobs, p, sa64, b, large=False)
        assert oinfo["ordinary"] == 8
        assert same_arrays(on.arrays, off.arrays)


def test_scores_beyond_32_bits():
    jobs = C.wide_score_jobs()
    for p in C.RUNS["wide_score"]:
        chains, info = chain(jobs, p, large=True)
        assert info["shared"] == len(jobs) and info["flagged"] == 0
        check("wide_score", p, chains)
    assert abs(int(chains.end_score[0])) > 1 << 32


def test_rounds():
    jobs = C.mixed_jobs()
    whole, info = chain(jobs)
    assert info["rounds"] == 1
    total = sum(C.ranks(s) for s in jobs if many.takes_shared_scan([x.encode("latin-1") for x in s]))
    b = many.Batch()
    b.option("RV_MANY_ROUND", total // 4)
    cut, cinfo = chain(jobs, batch=b)
    assert cinfo["rounds"] >= 3
    assert same_arrays(whole.arrays, cut.arrays)


def test_launches_do_not_grow_with_the_jobs():
    """10 jobs against 1000 copies of them: the same launches (both rounds hold more than 2048 and fewer than 2^22 ranks, as in the scan's test)"""
    import random
    rng = random.Random(6)
    jobs = [C.family(rng, ("indel", "snp")[i % 2], (2, 3)[i % 2], (150, 100)[i % 2]) for i in range(10)]
    few, finfo = chain(jobs)
    lots, linfo = chain(jobs * 1000)
    assert finfo["rounds"] == linfo["rounds"] == 1 and finfo["shared"] == 10 and linfo["shared"] == 10000
    assert finfo["launches"] == linfo["launches"], (finfo, linfo)
    for j in range(10):
        lens = [len(s) for s in jobs[j]]
        want = K.kchain_python(C.oracle_records(tuple(jobs[j]), 20), lens)
        assert (lots[9990 + j], int(lots.end_score[9990 + j])) == (few[j], int(few.end_score[j])) == want
        assert len(want[0]) > 0


def test_batch_reuse():
    jobs = [list(j) for j in C.mixed_jobs()[:30] if len(j) <= 64 and "\0" not in "".join(j)]
    b = many.Batch()
    first, _ = chain(jobs, batch=b)
    with pytest.raises(many.error):
        b.matches()
    b.scan(20, 2, "auto")
    m1 = b.matches()
    with pytest.raises(many.error):
        b.chains()
    b.kchain()
    assert same_arrays(first.arrays, b.chains())
    b.run(20, 2)
    an = b.anchors()
    with pytest.raises(many.error):
        b.chains()
    b.kchain()
    assert same_arrays(first.arrays, b.chains())
    b.scan(20, 2, "auto")
    assert same_arrays(m1, b.matches())
    b.run(20, 2)
    again = b.anchors()      # (the order of a job's anchors is the kernels', launch by launch: the jobs' counts and the lengths, sorted)
    assert np.array_equal(an[0], again[0]) and sorted(an[1].tolist()) == sorted(again[1].tolist())
    ref, _ = many.mums_many(jobs, toupper=False)
    assert same_arrays(ref.arrays, m1)


@pytest.mark.parametrize("name", sorted(C.recurse_inputs()))
def test_chain_recurse(name):
    with open(os.path.join(GOLD, "kchain_recurse.json")) as f:
        want = json.load(f)["inputs"][name]
    anchors, infos = K.chain_recurse(list(C.recurse_inputs()[name]), toupper=False, **C.RECURSE_PARAMS)
    assert [[l, [list(x) for x in mem], d] for l, mem, d in anchors] == want["anchors"]
    assert max(d for _, _, d in anchors) == want["maxdepth"] >= 2 and len(infos) >= 3
