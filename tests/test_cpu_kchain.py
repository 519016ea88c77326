"""CPU suite: `rv_kchain` (host C++, csrc/rv_kchain.hip) and `kchain.kchain_python` against tests/golden/kchain_vectors.json -- the reference's own
chain() (tools/gen_kchain_golden.py) -- path for path and score for score; what the file has to hold is asserted on the file itself; and
tests/golden/many_kchain.json / kchain_recurse.json are checked against the batches of tests/kchain_cases.py as they are generated today."""
import json
import os

import pytest

import kchain_cases as C
from helpers import GOLD
from reveal_amd import kchain as K


def load(name):
    with open(os.path.join(GOLD, name)) as f:
        return json.load(f)


CASES = load("kchain_vectors.json")["cases"]


def records(c):
    return [(r[0], r[1], tuple(zip(r[2::2], r[3::2]))) for r in c["records"]]      # [l, n, sample, pos, sample, pos, ..]


def want(c):
    return [(l, tuple(v), sc) for l, v, sc in c["path"]], c["end_score"]


def args(c):
    return c["maxmums"], c["wpen"], c["wscore"], c["gcmodel"]


def test_python_restatement_equals_the_reference():
    for i, c in enumerate(CASES):
        assert K.kchain_python(records(c), c["lens"], *args(c)) == want(c), (i, c["tag"])


@pytest.mark.parametrize("sa64", [False, True])
def test_rv_kchain_equals_the_reference(sa64):
    for i, c in enumerate(CASES):
        assert K.kchain_native(records(c), c["lens"], *args(c), sa64=sa64) == want(c), (i, c["tag"])


def full(c):
    return [r for r in c["records"] if r[1] == c["k"]]


def test_the_file_holds_what_the_tests_need():
    assert {c["k"] for c in CASES} >= {2, 3, 8, 16, 64}
    assert {c["gcmodel"] for c in CASES} == {"sumofpairs", "star-avg", "star-med"}
    ms = {len(full(c)) for c in CASES}
    assert 0 in ms and 1 in ms and max(ms) >= 200
    assert any(len(full(c)) < len(c["records"]) for c in CASES)      # records of fewer sequences, for the filter
    # the kd-order tie rule decides: the same ties decided by dimension 0 give another path
    decided = sum(1 for c in CASES if K.kchain_python(records(c), c["lens"], *args(c), tie="dim0")[0] != want(c)[0])
    assert decided >= 10, decided
    # the cap cuts through a run of equal lengths
    cut = 0
    for c in CASES:
        ls = sorted(r[0] for r in full(c))
        mm = c["maxmums"]
        if mm and len(ls) > mm and ls[len(ls) - mm - 1] == ls[len(ls) - mm]:
            cut += 1
    assert cut >= 5, cut
    # p1 stays the best predecessor of a node that has admissible candidates
    stays = 0
    for c in CASES:
        if c["tag"] != "p1_stays":
            continue
        path, _ = want(c)
        for l, v, sc in path:      # a node whose score is p1's own offer although another match ends in front of it in every sequence
            lens = c["lens"]
            begin = [sum(lens[:d]) + d for d in range(c["k"])]
            pts = [(r[0], tuple(sorted(r[3::2]))) for r in full(c)]
            pts = [(pl, tuple(p[d] - begin[d] for d in range(c["k"]))) for pl, p in pts]
            adm = [p for pl, p in pts if all(p[d] + pl <= v[d] for d in range(c["k"]))]
            if adm and sc == -c["wpen"] * K.gapcost(tuple([-1] * c["k"]), v, c["gcmodel"]):
                stays += 1
    assert stays >= 1
    wide = [c for c in CASES if c["wpen"] == 65536 and max([abs(c["end_score"])] + [abs(n[2]) for n in c["path"]]) > 1 << 32]
    assert len(wide) >= 3


def test_arguments():
    with pytest.raises(K.error):
        K.kchain_python([(5, 2, ((0, 1), (1, 14))), (3, 2, ((0, 7), (1, 20)))], [10, 10], gcmodel="nonsense")
    # no record, and records of fewer sequences only: the empty path and p1's offer to p2
    assert K.kchain_native([], [10, 14], wpen=3) == ([], -3 * 4) == K.kchain_python([], [10, 14], wpen=3)
    recs = [(5, 2, ((0, 1), (2, 30)))]
    assert K.kchain_native(recs, [10, 14, 12]) == K.kchain_python(recs, [10, 14, 12]) == ([], -K.gapcost((-1, -1, -1), (10, 14, 12)))


def test_level_jobs():
    # two nodes in a pair job at offsets (100, 200): gaps in front, between (one side only: dropped at minn = 2) and behind
    nodes = [(10, (105, 207)), (5, (115, 230))]
    got = K.level_jobs(nodes, (100, 200), (130, 250), [0, 1], 2)
    assert got == [([0, 1], [100, 200], [105, 207]), ([0, 1], [120, 235], [130, 250])]
    assert K.level_jobs(nodes, (100, 200), (130, 250), [0, 1], 1)[1] == ([1], [217], [230])


MANY = load("many_kchain.json")["runs"]


def test_many_kchain_json_is_consistent_with_the_batches():
    """every batch and parameter set of kchain_cases has its run in the file, a job for a job; and on the jobs a CPU test can afford, the Python
    restatement over the oracle's list of the job alone gives the file's chain"""
    assert set(MANY) == {C.run_key(b, p) for b in C.BATCHES for p in C.RUNS[b]}
    for b, jobs in C.BATCHES.items():
        for p in C.RUNS[b]:
            assert len(MANY[C.run_key(b, p)]) == len(jobs())
    jobs = C.mixed_jobs()
    assert 140 <= len(jobs) <= 160 and {len(j) for j in jobs} >= {2, 3, 8, 32, 64, 65}
    assert any("\0" in s for j in jobs for s in j)
    assert min(len(s) for j in jobs for s in j) >= 10 and max(len(s) for j in jobs for s in j) <= 1000
    sizes = set()
    for p in C.RUNS["mixed"][:1] + C.RUNS["mixed"][-3:-2]:
        gold = MANY[C.run_key("mixed", p)]
        for j in range(0, len(jobs), 2):
            seqs = jobs[j]
            path, end = K.kchain_python(C.oracle_records(tuple(seqs), p["minlength"]), [len(s) for s in seqs], p["maxmums"], p["wpen"], p["wscore"], p["gcmodel"])
            assert C.digest(path, end) == gold[j], (j, len(seqs))
            sizes.add(len(path))
    assert 0 in sizes and 1 in sizes and max(sizes) > 10      # jobs with no full match, with one, with a long chain


def test_recurse_json_reaches_depth_two():
    rec = load("kchain_recurse.json")["inputs"]
    assert set(rec) == set(C.recurse_inputs())
    for name, r in rec.items():
        assert r["maxdepth"] >= 2 and len(r["anchors"]) > 20, name
        assert max(a[2] for a in r["anchors"]) == r["maxdepth"]
