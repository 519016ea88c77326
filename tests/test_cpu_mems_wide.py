"""getmultimems of indices of more than 64 samples: the CPU restatement (oracle/reveal_oracle.c, which counts an interval's samples
in an array as reveal.c:261-290 does) against the reference's own C, where tests/test_gpu_mems_wide.py uses it as the expected value.
oracle/pin_oracle.py pins this pair at a handful of samples only."""
import pytest

from helpers import assemble, csr_tuples, oracle, synth


def family(L, k, seed, repeated=0):
    """k samples of L bases each; the last `repeated` of them verbatim copies of sample 0 (intervals with many members from few samples)"""
    seqs = [g.decode() for g in synth.genomes(L, k - repeated, seed=seed)]
    return seqs + [seqs[0]] * repeated


@pytest.mark.parametrize("k,L,repeated,sa64", [(70, 3000, 0, False), (70, 2500, 12, True), (130, 2000, 0, False), (130, 2000, 30, False)])
def test_restatement_equals_reference_at_wide_indices(k, L, repeated, sa64):
    from oracle import ref_ctypes
    if not ref_ctypes.available(sa64):
        pytest.skip("oracle/_ref is not built here")
    seqs = family(L, k, seed=5 + k, repeated=repeated)
    T, nsep, nodes = assemble(seqs)
    O = oracle(sa64)
    c = O.construct(T, nsep, k)
    R = ref_ctypes.Ref(sa64)
    tb_r = R.textbuf(T)
    SO = R.build_so(nsep, k, len(T))
    ri = R.view(tb_r, c["SA"], c["LCP"], nsep, k, SAi=c["SAi"], SO=SO)
    records = 0
    for minl, minn in ((15, 2), (12, 3), (20, k // 2), (12, k - repeated), (15, k), (4, 2)):
        ref = R.getmultimems(ri, minl, minn)
        mine = csr_tuples(*O.getmultimums(c["tbuf"], c["SA"], c["LCP"], c["SO"], nsep, k, minl, minn, mems=True))
        assert len(mine) == len(ref), (minl, minn)
        assert mine == ref, (minl, minn)
        records += len(ref)
    assert records > 100
