"""The run's tail under the cascade's levels: once the caller's result arrays are in use (rv_set_result_buffers: from a handle's second run on),
the anchors a batch of levels has completed leave for them on a side stream while the next batch runs, and the end of the run copies only what
is left (rv_cascade.hip send_known, rv_align.hip builtin_finish).  Anchors, statistics and final text equal the oracle's whatever the batch
size, when results grow, shrink or do not fit, and when an attempt whose anchors have already left is abandoned."""
import functools
import random

import pytest

from helpers import assemble, feed, oracle, synth

pytestmark = pytest.mark.gpu


def mod(sa64):
    from reveal_amd import reveallib, reveallib64
    return reveallib64 if sa64 else reveallib


def aset(a):
    l, off, pos = a[0], a[-2], a[-1]
    return sorted((int(l[k]), tuple(int(x) for x in pos[off[k]:off[k + 1]])) for k in range(len(l)))


def oracle_run(inputs, minl, sa64=False):
    T, nsep, nodes = assemble(inputs)
    O = oracle(sa64)
    ref = O.align_bench(O.construct(T, nsep, len(inputs)), nodes, minl, 2)
    return dict(anchors=aset(ref["anchors"]), T=ref["T"], stats=ref["stats"])


@functools.lru_cache(maxsize=None)
def synth_case(length, seed, sa64=False):
    inputs = [g.decode() for g in synth.genomes(length, 2, seed=seed)]
    return inputs, oracle_run(inputs, 20, sa64)


def run_and_check(idx, ref, minl=20):
    """construct() + align_builtin() on the handle; everything the run hands out against the oracle's.  -> cascade_info()"""
    idx.construct()
    got = idx.align_builtin(minl, 2)
    info = idx.cascade_info()
    assert aset(got["anchors"]) == ref["anchors"]
    assert idx.T.encode("latin-1") == ref["T"]
    assert got["stats"]["splits"] == ref["stats"]["nsplits"] and got["stats"]["steps"] == ref["stats"]["nsteps"]
    assert got["stats"]["anchored_bp"] == ref["stats"]["anchored_bp"]
    del got      # (the arrays go back to the handle: the next run delivers into them)
    return info


@pytest.mark.parametrize("sa64", [False, True])
@pytest.mark.parametrize("batch", [1, 3, 8])
def test_anchors_leave_under_the_levels(monkeypatch, batch, sa64):
    """2 x 300 kbp at 1 % SNP: more than eight levels, so every batch size sends more than one range.  The first run has no result arrays yet
    (today's tail), the following ones deliver into the arrays of the run before"""
    monkeypatch.setenv("RV_CASCADE_BATCH", str(batch))
    inputs, ref = synth_case(300_000, 5, sa64)
    idx = feed(mod(sa64).index(), inputs)
    for turn in range(3):
        info = run_and_check(idx, ref)
        assert info["done"] and info["levels"] > 8, info


@pytest.mark.parametrize("sa64", [False, True])
def test_results_that_grow_shrink_and_do_not_fit(monkeypatch, sa64):
    """one set of result arrays handed from handle to handle (the sequence of test_anchors_delivered_into_the_callers_arrays), a range at a time:
    the larger result does not fit the smaller one's arrays -- its first ranges have left for them before the run finds out"""
    monkeypatch.setenv("RV_CASCADE_BATCH", "1")
    big, small = synth_case(400_000, 21, sa64), synth_case(90_000, 22, sa64)
    idx = feed(mod(sa64).index(), small[0])
    for inp, ref in (small, small, big, big, small, small):
        idx2 = feed(mod(sa64).index(), inp)
        idx2.__dict__["_res_bufs"] = idx.__dict__.get("_res_bufs")
        idx.__dict__.pop("_res_bufs", None)
        idx._dll.rv_set_result_buffers(idx._h, None, 0, None, 0, None, 0)
        assert run_and_check(idx2, ref)["done"]
        idx = idx2


def _tandem_cases(seed, ncases, base_len, array_len):
    rng = random.Random(seed)
    for case in range(ncases):
        base = "".join(rng.choice("ACGT") for _ in range(base_len))
        unit = "".join(rng.choice("ACGT") for _ in range(rng.choice(array_len[0])))
        arr = unit * ((rng.choice(array_len[1]) if len(array_len[1]) > 1 else array_len[1][0]) // len(unit))

        def mutated(s, every):
            s = list(s)
            for p in range(rng.randint(0, every), len(s), every):
                s[p] = rng.choice("ACGT")
            return "".join(s)
        h = base_len // 2
        yield [base[:h] + mutated(arr, 97) + base[h:], base[:h] + mutated(arr, 89) + base[h:]]


def test_abandoned_attempts_deliver_nothing(monkeypatch):
    """the inputs of test_cascade_gives_up_cleanly and test_second_attempt_takes_what_the_leaf_kernel_cannot (tests/test_gpu_cascade.py), a level per
    batch and result arrays in use (the handle's second run): ranges have left before the attempt is dropped; what follows -- the level pipeline
    from the top, the interval cascade -- must deliver the oracle's anchors and text all the same"""
    monkeypatch.setenv("RV_CASCADE_DANGER", "0")
    monkeypatch.setenv("RV_CASCADE_BATCH", "1")
    gave_up = second = 0
    for inputs in list(_tandem_cases(3, 4, 30000, ([7, 23, 61], [6000]))) + list(_tandem_cases(12, 5, 40000, ([11, 23, 47], [1500, 2200, 3000]))):
        ref = oracle_run(inputs, 20)
        idx = feed(mod(False).index(), inputs)
        for turn in range(2):
            info = run_and_check(idx, ref)
        gave_up += (not info["done"]) and info["matches"] > 0
        second += info["done"] and info["rebuilt_ranks"] > 2048
    assert gave_up > 0 and second > 0, (gave_up, second)


def test_several_sequences_per_sample(tmp_path, monkeypatch):
    """contigs cut differently and shuffled (test_cascade_with_several_sequences_per_sample): the chain's anchors sit in front of the device's
    and leave with the first range"""
    monkeypatch.setenv("RV_CASCADE_BATCH", "1")
    rng = random.Random(17)
    base = "".join(rng.choice("ACGT") for _ in range(240000))
    var = "".join(rng.choice("ACGT") if rng.random() < 0.01 else c for c in base)

    def cut(s, k):
        at = sorted(rng.sample(range(200, len(s) - 200), k - 1))
        return [s[i:j] for i, j in zip([0] + at, at + [len(s)])]
    c1, c2 = cut(base, 5), cut(var, 6)
    rng.shuffle(c2)
    inputs = []
    for name, contigs in (("a.fa", c1), ("b.fa", c2)):
        with open(tmp_path / name, "w") as f:
            for k, s in enumerate(contigs):
                f.write(">c%d\n%s\n" % (k, s))
        inputs.append(str(tmp_path / name))
    ref = oracle_run(inputs, 20)
    idx = feed(mod(False).index(), inputs)
    for turn in range(3):
        info = run_and_check(idx, ref)
        assert info["done"] and info["subindices"] > 100, info
