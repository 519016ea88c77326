"""GPU suite: the chaining programme in device memory (csrc/rv_kchain_big.hip) -- `kchain.kchain_device` on the lists of tests/golden/kchain_big.json
(digests of the reference's own chain(), tools/gen_kchain_big_golden.py), `kchain_many` where the big path takes what the rounds' kernel gives back
or the scan runs the ordinary way, and `chain_recurse` with a top level above the kernel's cap."""
import json
import os
import random

import numpy as np
import pytest

import kchain_big_cases as B
import kchain_cases as C
from helpers import GOLD
from reveal_amd import kchain as K
from reveal_amd import many

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLD, "kchain_big.json")) as f:
    BIG = json.load(f)
with open(os.path.join(GOLD, "many_kchain.json")) as f:
    MANY = json.load(f)["runs"]

T = K.KCHAIN_BIG_TILE


def chain(jobs, p=C.P0, batch=None, large=None):
    return K.kchain_many([list(j) for j in jobs], p["minlength"], p["maxmums"], p["wpen"], p["wscore"], p["gcmodel"], toupper=False, batch=batch, large=large)


def same_arrays(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def n_full(seqs, minl=20):
    return sum(1 for r in C.oracle_records(tuple(seqs), minl) if r[1] == len(seqs))


@pytest.mark.parametrize("sa64", [False, True])
def test_golden_cases_one_by_one_and_in_one_call(sa64):
    b = many.Batch(sa64)
    lists = []
    for case in BIG["cases"]:
        recs, lens = B.build(case)
        lists.append((recs, lens))
        p = B.params(case)
        res, info = K.kchain_device([(recs, lens)], p["maxmums"], p["wpen"], p["wscore"], p["gcmodel"], sa64=sa64, batch=b, big_min=1)
        assert C.digest(*res[0]) == case["digest"], (case, res[0][0][:3], res[0][1])
        assert info["big"] == (1 if case["kept"] else 0) and info["host"] == 1 - info["big"] and info["lists"] == 1
        assert info["big_launches"] == (-(-(case["kept"] + 1) // T) if case["kept"] else 0)
    # all of them in ONE call: 1 .. 21 tiles, so that lists run out while others go on
    for p in (dict(maxmums=0, wpen=1, wscore=1, gcmodel="sumofpairs"), dict(maxmums=T + 1, wpen=3, wscore=1, gcmodel="star-med")):
        res, info = K.kchain_device(lists, p["maxmums"], p["wpen"], p["wscore"], p["gcmodel"], sa64=sa64, batch=b, big_min=1)
        full = [sum(1 for r in recs if r[1] == len(lens)) for recs, lens in lists]
        kept = [min(x, p["maxmums"]) if p["maxmums"] else x for x in full]
        assert info["big"] == sum(1 for x in kept if x) and info["big_launches"] == -(-(max(kept) + 1) // T)
        for case, (recs, lens), got in zip(BIG["cases"], lists, res):
            assert got == K.kchain_native(recs, lens, p["maxmums"], p["wpen"], p["wscore"], p["gcmodel"]), case
            if B.params(case) == p:
                assert C.digest(*got) == case["digest"]


def test_launches_count_the_tiles_not_the_lists():
    case = next(c for c in BIG["cases"] if c["tag"] == "random" and c["k"] == 2 and c["m"] == 3 * T + 5)
    one = B.build(case)
    p = B.params(case)
    few, finfo = K.kchain_device([one] * 2, p["maxmums"], p["wpen"], p["wscore"], p["gcmodel"], big_min=1)
    lots, linfo = K.kchain_device([one] * 20, p["maxmums"], p["wpen"], p["wscore"], p["gcmodel"], big_min=1)
    assert finfo["big"] == 2 and linfo["big"] == 20
    assert finfo["big_launches"] == linfo["big_launches"] == 4
    assert all(C.digest(*r) == case["digest"] for r in few + lots)


def test_flagged_jobs_come_back_through_the_big_path():
    """RV_KCHAIN_CAP = 0 flags every shared job with a record; with RV_KCHAIN_BIG_MIN = 1 each of them is chained in device memory"""
    jobs = C.mixed_jobs()
    b = many.Batch()
    b.option("RV_KCHAIN_CAP", 0)
    b.option("RV_KCHAIN_BIG_MIN", 1)
    for p in (C.P0, C.RUNS["mixed"][3]):
        b.option("RV_MANY_KCHAIN_BIG", 1)
        big, info = chain(jobs, p, batch=b)
        b.option("RV_MANY_KCHAIN_BIG", 0)
        host, hinfo = chain(jobs, p, batch=b)
        gold = MANY[C.run_key("mixed", p)]
        for j, want in enumerate(gold):
            assert C.digest(big[j], big.end_score[j]) == want, (p, j)
        assert same_arrays(big.arrays, host.arrays)
        shared = [many.takes_shared_scan([x.encode("latin-1") for x in s]) for s in jobs]
        assert info["flagged"] == hinfo["flagged"] == sum(1 for s, sh in zip(jobs, shared) if sh and n_full(s, p["minlength"]) > 0) > 0
        assert hinfo["big"] == 0 and hinfo["big_launches"] == 0
        assert info["big"] >= info["flagged"] and info["big_launches"] > 0      # (the flagged ones, and the ordinary job with a NUL byte where it has a match)
        assert info["big"] <= info["flagged"] + info["ordinary"]


def test_natural_entry_at_defaults():
    """lists above the cap of the rounds' kernel, flagged by it (large class) or from the ordinary path: both reach the big path with no switch"""
    rng = random.Random(41)
    jobs = [C.blocks_job(rng, 2, 1100), C.blocks_job(rng, 3, 1030)]
    assert [n_full(s) for s in jobs] == [1100, 1030]
    want = [K.kchain_native(C.oracle_records(tuple(s), 20), [len(x) for x in s]) for s in jobs]
    b = many.Batch()
    b.option("RV_MANY_SCAN_LARGE_MIN", 1)
    on, info = chain(jobs, batch=b, large=True)
    assert info["shared"] == 2 and info["flagged"] == 2 and info["big"] == 2
    off, oinfo = chain(jobs, batch=b, large=False)
    assert oinfo["ordinary"] == 2 and oinfo["flagged"] == 0 and oinfo["big"] == 2
    assert info["big_launches"] == oinfo["big_launches"] == -(-1101 // T)
    for res in (on, off):
        for j in range(2):
            assert (res[j], int(res.end_score[j])) == want[j]


def test_member_cap_at_defaults():
    jobs = C.member_jobs()
    b = many.Batch()
    b.option("RV_MANY_SCAN_LARGE_MIN", 1)
    chains, info = chain(jobs, batch=b, large=True)
    for j, want in enumerate(MANY[C.run_key("members", C.P0)]):
        assert C.digest(chains[j], chains.end_score[j]) == want
    assert info["shared"] == 2 and info["flagged"] == 1
    assert info["big"] == (1 if 513 >= K.KCHAIN_BIG_MIN else 0)


def test_chain_recurse_above_the_cap():
    seqs = list(B.recurse_big_input())
    want = BIG["recurse"]
    assert n_full(seqs) == want["top"] > K.KCHAIN_CAP
    anchors, infos = K.chain_recurse(seqs, toupper=False, **C.RECURSE_PARAMS)
    assert [[l, [list(x) for x in mem], d] for l, mem, d in anchors] == want["anchors"]
    assert max(d for _, _, d in anchors) == want["maxdepth"]
    assert infos[0]["big"] == 1 and infos[0]["big_launches"] == -(-(want["top"] + 1) // T)
