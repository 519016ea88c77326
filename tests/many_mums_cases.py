"""inputs of the mums_many tests (tests/test_cpu_many_mums.py checks them, tests/test_gpu_many_mums.py uses them): three batches built from
the generators of many_cases / many_multi_cases / many_wide_cases, the corner jobs of the scan kernels, five jobs for the ordinary path, and
the checker -- the CPU oracle on the job ALONE (helpers.assemble + Oracle.construct + Oracle.getmums / Oracle.getmultimums), never the ordinary
path and never mums_many.  Sequences are str and are scanned as given (toupper=False): lower case survives.  Deterministic."""
import bisect
import functools
import random

import many_cases as mc
import many_multi_cases as mm
import many_wide_cases as mw

MAX_RANKS = 2048      # ranks (sum of lengths + k) of the largest job the shared launches take
MAX_K = 64            # ... and its sequences


def ranks(seqs):
    return sum(len(s) for s in seqs) + len(seqs)


def pair_batch():
    """44 pair jobs, four of every class of many_cases"""
    return [list(p) for _, p in mc.class_jobs(4)]


def multi_batch():
    """45 families of k = 3, 4, 5, 8, 16 over the nine classes of many_multi_cases"""
    return [fam for _, _, fam in mm.class_jobs(5)]


def wide_batch():
    """one family for each k of 17, 24, 32, 33, 48, 64"""
    return [fam for _, _, fam in mw.class_jobs(1)]


# a job of four short sequences whose last rank closes three nested intervals: the only suffixes that begin with T are TA$ < TGA$ < TGCA$ < TGCCA$,
# one per sample, and they end the order; the thread of the last rank emits (3, n=2), (2, n=3) and (1, n=4) -- test_cpu_many_mums checks it on the oracle
NESTED_LAST = ["TGA", "TGCA", "TGCCA", "TA"]


def corner_jobs(seed=17):
    """-> [(name, [seq, ..])]: the smallest shapes at which the scan kernels can go wrong"""
    rng = random.Random(seed)
    x = mc.rnd(rng, 25)
    out = [
        ("two_single_bases", ["A", "C"]),
        ("two_equal_single_bases", ["G", "G"]),
        ("identical_pair", [x + "ACGTTGCA"] * 2),
        ("identical_five", [mc.rnd(rng, 40)] * 5),
        ("tandem_family", mm.make_family("tandem", random.Random(seed + 1), 4)),
        # the only match lies at job-local position 0 (BWT '$' for "nothing in front"); the partner is the first thing of its sequence too, so
        # the pair is maximal through '$' alone
        ("match_at_position_0", [x + "A" + mc.rnd(rng, 30, "AC"), x + "G" + mc.rnd(rng, 30, "GT")]),
        ("match_at_position_0_inner", [x + "A" + mc.rnd(rng, 30, "AC"), mc.rnd(rng, 12, "GT") + x + "G" + mc.rnd(rng, 12, "GT")]),
        # equal characters in front of both copies: maximal only because that character is N / lower case
        ("maximal_through_N", ["CCA" + "N" + x + "A", "GGT" + "N" + x + "T"]),
        ("maximal_through_lower", ["CCA" + "g" + x + "A", "GTT" + "g" + x + "T"]),
        ("not_maximal", ["CCA" + "G" + x + "A", "TTT" + "G" + x + "T"]),      # (the match is one base longer: the control of the two above)
        ("maximal_through_sep_three", [mc.rnd(rng, 30, "AC"), x + "A", x + "T"]),      # both copies begin their sequence: '$' in front of both
        ("nested_last_rank", list(NESTED_LAST)),
    ]
    for n in (511, 512, 513, 2047, 2048):      # the wavefront and workgroup classes of the build, the largest shared job
        out.append(("pair_ranks_%d" % n, mm.sized_job(rng, 2, n)))
        out.append(("three_ranks_%d" % n, mm.sized_job(rng, 3, n)))
    for k in (2, 3, 16, 17, 32, 33, 63, 64):
        out.append(("k%d" % k, mm.sized_job(rng, k, k * 31, 0.02)))
    return out


def ordinary_jobs(seed=23):
    """-> [(name, [seq, ..])]: five jobs the shared launches do not take"""
    rng = random.Random(seed)
    a = mc.rnd(rng, 1400)
    nul = mc.rnd(rng, 60)
    return [
        ("pair_ranks_2049", mm.sized_job(rng, 2, 2049)),
        ("pair_ranks_3000", mm.sized_job(rng, 2, 3000)),
        ("k65", mm.sized_job(rng, 65, 65 * 31, 0.02)),
        ("nul_byte", [nul, nul[:30] + "\0" + nul[31:]]),
        ("three_by_1000", [mc.mutate(rng, a[:1000], 0.01) for _ in range(3)]),
    ]


# ---- the checker ----
@functools.lru_cache(maxsize=None)
def _index(seqs):
    from helpers import assemble, oracle
    T, nsep, _ = assemble(list(seqs), toupper=False)
    c = oracle(False).construct(T, nsep, len(seqs))
    return T, nsep, c


@functools.lru_cache(maxsize=None)
def _oracle(seqs, kind, minl, minn):
    from helpers import csr_tuples, oracle
    T, nsep, c = _index(seqs)
    O = oracle(False)
    k = len(seqs)
    if kind == "mums" or (kind == "auto" and k == 2):
        l, a, b = O.getmums(c["tbuf"], c["SA"], c["LCP"], nsep, minl)
        return tuple((int(l[i]), 2, ((0, int(a[i])), (bisect.bisect_left(nsep, int(b[i])), int(b[i])))) for i in range(len(l)))
    return tuple(csr_tuples(*O.getmultimums(c["tbuf"], c["SA"], c["LCP"], c["SO"], nsep, k, minl, minn)))


def oracle_matches(seqs, kind="auto", minl=20, minn=2):
    """the list of ONE job, alone, as records (l, n, ((sample, pos), ..)) in the oracle's emission order; a getmums record is
    (l, 2, ((0, a), (sample of b, b))).  Computed once per (job, parameters) and shared; nobody changes what it returns.  The numbers do not
    depend on the width of the library's suffix array, so the 32-bit oracle checks both libraries."""
    return _oracle(tuple(seqs), kind, int(minl), int(minn if not (kind == "mums" or (kind == "auto" and len(seqs) == 2)) else 2))


def oracle_arrays(seqs):
    _, _, c = _index(tuple(seqs))
    return c["SA"], c["LCP"]


def closing_ranks(seqs, recs):
    """the rank at which each record's interval ends: the largest rank of its members"""
    _, _, c = _index(tuple(seqs))
    return [max(int(c["SAi"][p]) for _, p in mem) for _, _, mem in recs]


def follows_order_rule(seqs, recs):
    """closing rank ascending, then l descending -- strictly: no two records of a job share both"""
    key = [(u, -l) for u, (l, _, _) in zip(closing_ranks(seqs, recs), recs)]
    return all(key[i] < key[i + 1] for i in range(len(key) - 1))


def job_records(arrays, j):
    """job j of a CSR (first, l, n, off, so, pos) as records (l, n, ((sample, pos), ..)), in the order given"""
    first, l, n, off, so, pos = arrays
    return tuple((int(l[k]), int(n[k]), tuple((int(so[q]), int(pos[q])) for q in range(int(off[k]), int(off[k + 1])))) for k in range(int(first[j]), int(first[j + 1])))
