"""getmultimems (rv_mems.hip) on indices of more than 64 samples, where the sample census of an interval no longer fits one 64-bit
mask: a thread keeps it in 2 or 4 words (up to 256 samples), the wavefront machine in an LDS bitmap, and beyond 256 samples every run
goes to the wavefront machine.  Expected value everywhere: the CPU restatement, which counts samples in an array like reveal.c:261-290
(tests/test_cpu_mems_wide.py pins it against the reference's own C at these widths).  Equality is exact: same records, same order."""
import random

import pytest

from helpers import assemble, csr_tuples, feed, oracle, synth

pytestmark = pytest.mark.gpu


def mod(sa64):
    from reveal_amd import reveallib, reveallib64
    return reveallib64 if sa64 else reveallib


def family(L, k, seed=42, snp=0.01):
    return [g.decode() for g in synth.genomes(L, k, seed=seed, snp=snp)]


class Pair:
    """the oracle's arrays and the GPU index of the same inputs"""

    def __init__(self, seqs, sa64=False):
        self.k = len(seqs)
        self.T, self.nsep, _ = assemble(seqs)
        self.O = oracle(sa64)
        self.c = self.O.construct(self.T, self.nsep, self.k)
        self.idx = feed(mod(sa64).index(), seqs)
        self.idx.construct()

    def ref(self, minl, minn):
        c = self.c
        return csr_tuples(*self.O.getmultimums(c["tbuf"], c["SA"], c["LCP"], c["SO"], self.nsep, self.k, minl, minn, mems=True))

    def check(self, minl, minn, nonempty=True):
        ref = self.ref(minl, minn)
        got = self.idx.getmultimems(minlength=minl, minn=minn)
        assert len(got) == len(ref), (self.k, minl, minn, len(got), len(ref))
        assert got == ref, (self.k, minl, minn)
        if nonempty:
            assert len(ref) > 0, (self.k, minl, minn)      # an empty list must not pass for agreement
        return ref


# 1. families just over each boundary of the census: a second word, config 5's shape, a third word, past the registers (and past
#    what 8 bits name).  n stays around 2-3 x 10^5.  Every sample also holds one copy of a 60-mer at a place of its own, so that
#    minn = nsamples has records to compare however far the samples have drifted apart
@pytest.mark.parametrize("k,L,minl,snp,sa64", [
    (65, 4500, 16, 0.01, False), (70, 4200, 12, 0.01, False), (70, 4200, 14, 0.003, True), (100, 3000, 20, 0.003, False),
    (129, 2300, 15, 0.01, False), (130, 2300, 12, 0.003, False), (130, 2300, 18, 0.003, True), (257, 800, 14, 0.003, False),
    (300, 700, 16, 0.003, False),
])
def test_families_over_each_boundary(k, L, minl, snp, sa64):
    rng = random.Random(k)
    seqs = family(L, k, seed=k, snp=snp)
    u = "".join(rng.choice("ACGT") for _ in range(60))
    for s in range(k):
        q = rng.randrange(L); seqs[s] = seqs[s][:q] + u + seqs[s][q:]
    p = Pair(seqs, sa64)
    top = -1
    for minn in (2, 3, k // 2, k):
        ref = p.check(minl, minn)
        top = max(top, max(so for _, _, spd in ref for so, _ in spd))
    # 5. the samples come out with their true ids, beyond 63 and beyond 255
    assert top == k - 1


# 2. the `continue` of reveal.c:340-342 with a wide census: intervals with many members from fewer than minn samples, inside intervals
#    of minn samples and more (whose left bound the exit changes)
def quirk_inputs(name):
    rng = random.Random(7)
    if name == "repeated_samples":              # sample 0 holds segments of itself three times, and samples 80-99 are all equal to it
        seqs = family(3000, 80, seed=21)
        v = seqs[0]
        for _ in range(6):
            q = rng.randrange(len(v) - 300); u = v[q:q + 200]
            for _ in range(2):
                q = rng.randrange(len(v)); v = v[:q] + u + v[q:]
        return [v] + seqs[1:] + [v] * 20
    if name in ("private_copies", "private_copies_beyond_256"):
        # a few samples, spread over the census words, each hold 8 more copies of 300-mers of the family
        wide = name != "private_copies"
        k, L = (300, 800) if wide else (100, 3000)
        seqs = family(L, k, seed=22)
        for _ in range(5):
            q = rng.randrange(L - 400); u = seqs[0][q:q + 300]
            for s in ((10, 70, 200, 299) if wide else (10, 70, 71, 99)):
                v = seqs[s]
                for _ in range(8):
                    q = rng.randrange(len(v)); v = v[:q] + u + v[q:]
                seqs[s] = v
        return seqs
    raise KeyError(name)


@pytest.mark.parametrize("name,minl,minn", [
    ("repeated_samples", 14, 85), ("private_copies", 12, 3), ("private_copies", 12, 10), ("private_copies", 16, 50),
    ("private_copies_beyond_256", 12, 3), ("private_copies_beyond_256", 14, 150),
])
def test_continue_quirk_with_a_wide_census(name, minl, minn):
    p = Pair(quirk_inputs(name))
    ref = p.check(minl, minn)
    # the input exercises the quirk only if the reference's list is not just its minn = 2 list filtered afterwards
    loose = [r for r in p.ref(minl, 2) if r[1] >= minn]
    assert ref != loose, "no interval of minn samples lost members through the `continue`: pick another input"


# 3. runs for the wavefront machine at a wide index: long (beyond 2048 ranks) and deep (beyond a thread's stack)
@pytest.mark.parametrize("k,L,sa64", [(72, 1500, False), (90, 1200, True), (140, 800, False), (260, 400, False)])
def test_long_and_deep_runs_at_a_wide_index(k, L, sa64):
    rng = random.Random(1000 + k)
    rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))
    seqs = family(L, k, seed=k)
    a, b, c = k - 1, k // 2, 66                                     # samples of the second census word and beyond
    at = rng.randrange(L)
    seqs[a] = seqs[a][:at] + "A" * 5000 + seqs[a][at:]              # a homopolymer: one run, as deep as it is long
    at = rng.randrange(L)
    seqs[b] = seqs[b][:at] + rnd(7) * 400 + seqs[b][at:]            # a tandem array
    at = rng.randrange(L)
    seqs[c] = seqs[c][:at] + "N" * 50 + "T" * 700 + seqs[c][at:]
    p = Pair(seqs, sa64)
    for minl, minn in ((5, 2), (3, k // 2), (6, k), (1, 2), (1, 3), (25, 2)):
        p.check(minl, minn)


# 4. the boundary itself: 64 samples (the unchanged one-word forms) and the same with a 65th
def test_the_boundary_itself():
    seqs = family(4500, 65, seed=64, snp=0.002)
    for part in (seqs[:64], seqs):
        p = Pair(part)
        for minl, minn in ((16, 2), (13, len(part) // 2), (16, len(part))):
            p.check(minl, minn)


def test_sample_ids_above_255_are_named():
    p = Pair(family(600, 300, seed=300))
    ref = p.check(16, 2)
    assert max(so for _, _, spd in ref for so, _ in spd) == 299
