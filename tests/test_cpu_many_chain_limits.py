"""The limits fixture of the five device pickers (tests/many_chain_limits_cases.py), without a device: the job list has the ranks and the k it states, the
golden file (tests/golden/many_chain_limits.json: `rem.align` on the reference's own index, tools/gen_many_chain_limits_golden.py) matches the list and is
consistent in itself, conditions (a) - (e) that make the file a test of the weight bounds and of the position fields hold -- and the generator's
condition function rejects a doctored document --, and the admission rule says yes for every job and set except the `over` set and the jobs of 2^17 + 1
ranks."""
import copy
import os
import sys

import pytest

import many_chain_limits_cases as lm
import many_multi_cases as mm
from helpers import oracle  # noqa: F401  (puts the repository root on sys.path)
from reveal_amd import many

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))

ALL_ON = dict(chain=True, chain_multi=True, chain_wide=True, chain_large=True, chain_large_multi=True)


def as_bytes(fam):
    return [s.upper().encode() for s in fam]


@pytest.fixture(scope="module")
def loaded():
    return lm.load_golden()


def test_the_jobs_have_the_ranks_and_the_k_they_state():
    for cls in lm.CLASSES:
        jobs = lm.jobs(cls)
        assert jobs == lm.jobs(cls) and 10 <= len(jobs) <= 16, cls
        nfar = len(lm.FAR[cls])
        nbig = lm.BIG_JOBS if cls in lm.LARGE_CLASSES else 0
        far = jobs[:nfar - nbig] + jobs[len(jobs) - nbig:]
        assert [c for c, _ in far] == ["far-swapped" if spec[6] else "far" for spec in lm.FAR[cls]]
        assert [(len(f), mm.ranks(f)) for _, f in far] == [(spec[0], spec[1]) for spec in lm.FAR[cls]]
        assert sum(c == "far-swapped" for c, _ in jobs) == 2
        assert 4 <= len(jobs) - nfar == lm.N_NEIGHBOURS[cls] <= 6
        assert [lm.is_big(cls, j) for j in range(len(jobs))] == [False] * (len(jobs) - nbig) + [True] * nbig
        # the far member is the longest by far, the first sequence of some jobs and the last of others
        at = [max(range(len(f)), key=lambda q: len(f[q])) for _, f in far]
        assert at == [0 if spec[2] else spec[0] - 1 for spec in lm.FAR[cls]] and len(set(spec[2] for spec in lm.FAR[cls])) == 2
        for (_, f), q in zip(far, at):
            assert len(f[q]) > 2 * max(len(s) for x, s in enumerate(f) if x != q)
        ks = {len(f) for _, f in jobs}
        ranks = [mm.ranks(f) for _, f in jobs]
        if cls in lm.LARGE_CLASSES:
            assert ranks[-3:] == [lm.TOP, lm.TOP, lm.TOP + 1] == [many.CHAIN_LARGE_RANKS] * 2 + [many.CHAIN_LARGE_RANKS + 1]
            assert all(2100 <= r <= 9000 for r in ranks[:-3])
            assert [len(f) for _, f in jobs[-3:]] == ([2] * 3 if cls == "chain_large" else [16] * 3)
            first = [max(range(len(f)), key=lambda q: len(f[q])) == 0 for _, f in jobs[-3:-1]]
            assert first == [True, False]                 # 2^17 ranks with the long sequence first, and with it last
            assert all(len(max(f, key=len)) > 1 << 16 for _, f in jobs[-3:])
            assert len(lm.fillers(cls)) + 2 >= (many.CHAIN_LARGE_MIN if cls == "chain_large" else many.CHAIN_LARGE_MULTI_MIN)
        else:
            assert max(ranks) == many.LEAF_RANKS and sum(r == many.LEAF_RANKS for r in ranks) >= 2
        assert ks == {2} if cls in ("chain", "chain_large") else (ks >= {3, 16} and max(ks) <= 16) if cls in ("chain_multi", "chain_large_multi") else (ks >= {17, 64} and min(ks) >= 17)
        if cls in ("chain_multi", "chain_wide"):
            lo, hi = (3, 16) if cls == "chain_multi" else (17, 64)
            assert {len(f) for _, f in jobs if mm.ranks(f) == many.LEAF_RANKS} >= {lo, hi}


def test_the_sets_stand_at_the_bounds_of_the_classes():
    assert [lm.wmax(cls) for cls in lm.CLASSES] == [65536, 1024, 1024, 1024, 512]
    assert [lm.wmax(cls) for cls in lm.CLASSES] == [many.CHAIN_WMAX, many.CHAIN_MULTI_WMAX, many.CHAIN_MULTI_WMAX, many.CHAIN_MULTI_WMAX, many.CHAIN_LARGE_MULTI_WMAX]
    for cls in lm.CLASSES:
        W = lm.wmax(cls)
        got = [(n, kw.get("wscore", 1), kw.get("wpen", 1), kw.get("gcmodel", "sumofpairs")) for n, kw in lm.sets(cls)]
        assert got == [("default", 1, 1, "sumofpairs"), ("wmax", W, W, "sumofpairs"), ("pen-max", 1, W, "sumofpairs"), ("score-max", W, 1, "sumofpairs"),
                       ("score-nopen", W, 0, "sumofpairs"), ("wmax-avg", W, W, "star-avg"), ("wmax-med", W, W, "star-med"), ("over", W + 1, W + 1, "sumofpairs")]
        assert all(kw["minlength"] == (5 if cls == "chain_wide" else 20) for _, kw in lm.sets(cls))
        assert all(dict(kw, **lm.BIG) == kb for (_, kw), (_, kb) in zip(lm.sets(cls), lm.sets(cls, big=True)))


def test_what_the_admission_rule_says_for_every_job_and_set():
    """yes for everything except the `over` set and the jobs of 2^17 + 1 ranks, and only with the class' own switch"""
    for cls in lm.CLASSES:
        jobs = lm.jobs(cls)
        for j, (c, fam) in enumerate(jobs):
            over_size = mm.ranks(fam) > many.CHAIN_LARGE_RANKS
            assert over_size == (cls in lm.LARGE_CLASSES and j == len(jobs) - 1)
            for name, kw in lm.sets(cls, big=lm.is_big(cls, j)):
                args = lm.picker_args(kw)
                want = name != "over" and not over_size
                assert many.takes_shared_launch(as_bytes(fam), picker=args, minlength=kw["minlength"], **lm.switch(cls)) == want, (cls, j, name)
                assert many.takes_shared_launch(as_bytes(fam), picker=args, minlength=kw["minlength"], **ALL_ON) == want, (cls, j, name)
                off = dict(ALL_ON, **{cls: False})
                assert not many.takes_shared_launch(as_bytes(fam), picker=args, minlength=kw["minlength"], **off), (cls, j, name)
        if cls in lm.LARGE_CLASSES:
            # rem.align's default seedsize and maxmums do not admit a job of 2^17 ranks; the fillers are admitted under the big sets
            assert not many.takes_shared_launch(as_bytes(jobs[-3][1]), picker=lm.picker_args(lm.sets(cls)[1][1]), **lm.switch(cls))
            for name, kw in lm.sets(cls, big=True)[:-1]:
                assert all(many.takes_shared_launch(as_bytes(f), picker=lm.picker_args(kw), **lm.switch(cls)) for f in lm.fillers(cls))


def test_golden_file_matches_the_job_list_and_is_self_consistent(loaded):
    """per class and set one result per job; the anchors of a job lie inside its sequences, one member per sequence at most, equal text under every
    member, disjoint on every sequence, and the upper-cased text lower-cased over them is the recorded final text; the recorded positions are the
    anchors' own"""
    golden, extremes = loaded
    for cls in lm.CLASSES:
        jobs = lm.jobs(cls)
        top = [[-1] * len(f) for _, f in jobs]
        for name in lm.SET_NAMES:
            assert len(golden[cls][name]) == len(jobs)
            for j, (_, fam) in enumerate(jobs):
                anchors, sha = golden[cls][name][j]
                text = bytearray(("".join(s.upper() + "$" for s in fam)).encode())
                beg = lm.begins_of(fam)
                assert anchors == sorted(anchors)
                covered = bytearray(len(text))
                for l, pos in anchors:
                    smp = [max(q for q in range(len(beg)) if beg[q] <= p) for p in pos]
                    assert l >= 1 and 2 <= len(pos) <= len(fam) and len(set(smp)) == len(smp), (cls, name, j)
                    for p, q in zip(pos, smp):
                        assert p + l <= beg[q] + len(fam[q]) and text[p:p + l] == text[pos[0]:pos[0] + l], (cls, name, j)
                        assert not any(covered[p:p + l]), (cls, name, j, "not disjoint")
                        covered[p:p + l] = b"\1" * l
                for l, pos in anchors:
                    for p in pos:
                        text[p:p + l] = text[p:p + l].lower()
                assert lm.sha(bytes(text)) == sha, (cls, name, j)
                top[j] = [max(a, b) for a, b in zip(top[j], lm.relative_positions(fam, anchors))]
        ext = extremes[cls]
        assert ext["job_positions"] == top
        assert sorted(ext["score"]) == sorted(ext["penalty"]) == sorted(lm.SET_NAMES)
        assert ext["penalty"]["score-nopen"] == 0 and all(ext["penalty"][n] > 0 for n in lm.SET_NAMES if n != "score-nopen")
    assert os.path.getsize(lm.GOLDEN) < 256 * 1000


def results_of(golden):
    return {cls: {n: list(golden[cls][n]) for n in lm.SET_NAMES} for cls in lm.CLASSES}


def test_the_fixture_conditions_hold_in_the_file(loaded):
    """conditions (a) - (e) of tools/gen_many_chain_limits_golden.py from the file, and spelled out"""
    import gen_many_chain_limits_golden as gen
    golden, extremes = loaded
    assert gen.conditions(lm, results_of(golden), extremes) == []
    changed = {}
    for cls in lm.CLASSES:
        res, ext = golden[cls], extremes[cls]
        assert res["wmax"] == res["default"] and res["over"] == res["default"], cls                                   # (a)
        assert sum(a != b for a, b in zip(res["pen-max"], res["default"])) >= 3, cls                                  # (b)
        changed[cls] = sum(a != b for a, b in zip(res["score-max"], res["default"]))
        top = max(ext["score"]["wmax"], ext["score"]["pen-max"])                                                       # (d)
        assert top >= dict(chain=1 << 26, chain_multi=1 << 22, chain_wide=1 << 24, chain_large=1 << 26, chain_large_multi=1 << 29)[cls], (cls, top)
        assert top < 1 << 31                  # what the kernels' header comments derive
    assert sum(changed.values()) >= 5 and sum(v > 0 for v in changed.values()) >= 3, changed                            # (c)
    assert max(extremes["chain_large_multi"]["penalty"][n] for n in ("wmax", "pen-max")) >= 1 << 28
    pos = {cls: extremes[cls]["job_positions"] for cls in lm.CLASSES}                                                    # (e)
    on0 = [j for j, p in enumerate(pos["chain_large"]) if p[0] >= 1 << 16]
    on1 = [j for j, p in enumerate(pos["chain_large"]) if p[1] >= 1 << 16]
    assert on0 and on1 and set(on0) != set(on1)
    assert any(p[0] >= 1 << 16 for p in pos["chain_large_multi"]) and any(len(p) == 16 and p[15] >= 1 << 16 for p in pos["chain_large_multi"])
    assert any(p[-1] >= 1024 for p in pos["chain_multi"]) and any(p[-1] >= 1024 for p in pos["chain_wide"])
    # the positions of the pairs of 2^17 ranks set bit 16 and stay inside 17 bits
    assert all(1 << 16 <= max(p) < 1 << 17 for cls in lm.LARGE_CLASSES for p in pos[cls][-3:])


def test_the_condition_function_rejects_a_doctored_document(loaded):
    import gen_many_chain_limits_golden as gen
    golden, extremes = loaded
    res = results_of(golden)

    def failures(results=res, ext=extremes):
        return " | ".join(gen.conditions(lm, results, ext))

    other = ([(1, (0, 1))], "0" * 64)
    assert "(a) chain: set over differs" in failures(dict(res, chain=dict(res["chain"], over=[other] + res["chain"]["over"][1:])))
    assert "(a) chain_wide: set wmax differs" in failures(dict(res, chain_wide=dict(res["chain_wide"], wmax=[other] + res["chain_wide"]["wmax"][1:])))
    assert "(b) chain_large: pen-max changes only 0" in failures(dict(res, chain_large=dict(res["chain_large"], **{"pen-max": res["chain_large"]["default"]})))
    same = {cls: dict(res[cls], **{"score-max": res[cls]["default"]}) for cls in lm.CLASSES}
    assert "(c) score-max changes" in failures(same)
    for cls in lm.CLASSES:
        low = copy.deepcopy(extremes)
        low[cls]["score"]["wmax"] = low[cls]["score"]["pen-max"] = gen.SCORE_MIN[cls] - 1
        assert "(d) %s: the largest |score|" % cls in failures(ext=low)
    low = copy.deepcopy(extremes)
    low["chain_large_multi"]["penalty"]["wmax"] = low["chain_large_multi"]["penalty"]["pen-max"] = (1 << 28) - 1
    assert "(d) chain_large_multi: the largest penalty product" in failures(ext=low)
    for cls, what in (("chain_large", "path 1"), ("chain_large_multi", "last sample of a job of 16"), ("chain_multi", "last sample"), ("chain_wide", "last sample")):
        low = copy.deepcopy(extremes)
        low[cls]["job_positions"] = [p[:-1] + [min(p[-1], 1023)] for p in low[cls]["job_positions"]]
        low[cls]["positions"] = [max(p[q] for p in low[cls]["job_positions"] if q < len(p)) for q in range(len(low[cls]["positions"]))]
        got = failures(ext=low)
        assert "(e) %s" % cls in got and what in got, (cls, got)
    low = copy.deepcopy(extremes)
    low["chain_large"]["job_positions"] = [[min(p[0], 65535), p[1]] for p in low["chain_large"]["job_positions"]]
    low["chain_large"]["positions"][0] = max(p[0] for p in low["chain_large"]["job_positions"])
    assert "(e) chain_large: no anchor at 2^16 or beyond on path 0" in failures(ext=low)
    low = copy.deepcopy(extremes)
    low["chain"]["positions"][0] += 1
    assert "(e) chain: positions is not the maximum" in failures(ext=low)


def test_the_golden_file_regenerates(loaded):
    import gen_many_chain_limits_golden as gen
    import pin_oracle as P
    refmod = P.load_refmod(False)
    if refmod is None:
        pytest.skip("oracle/_ref/reveallib.so not built (make -C oracle refmod needs the reference's sources)")
    golden, extremes = loaded
    for cls in lm.CLASSES:
        res, ext = gen.run_class(lm, cls, refmod)
        assert res == golden[cls], cls
        assert ext == extremes[cls], cls
