"""inputs of the capacity tests (tests/test_cpu_dense_cases.py pins the generator against the oracle, tests/test_gpu_capacity.py uses it):
small texts on which the lists that the scans fill by atomics overflow the capacities a fresh handle starts with, so that the retry of
each driver runs -- and a few repetitive ones for the lists that no small text overflows, which the tests reach through RV_CAP_LIMIT.
Deterministic: every text comes from numpy.random.default_rng(seed).integers, nothing else.

The capacities a fresh handle starts with (reveal_amd/csrc, m = ranks of the level, n = ranks of the index):
  pair scan, overflow buffer     4096 records + DBuf's growth margin            rv_api.hip rv_run_pair_scan, rv_cascade.hip rv_cascade_run
  pair scan, output list         max(4096, m / 64) records + the margin - header  (the same two drivers)
  pair scan, slots               16 per tile of 1024 ranks (RV_PAIR_SLOTS, RV_PAIR_TILE): what a tile holds beyond them goes to the overflow buffer
  first host copy of a level     scan_guess = 4096 records on a fresh handle, then the previous level's count + 1/16 + 64
  multi scan, records            max(4096, m / 32) + the margin                 rv_api.hip rv_run_multi_scan
  multi scan, members            max(8192, m / 8) + the margin
  multi picker, candidates       max(65536, m / 64) over 64 regions             rv_api.hip rv_run_multi_pick
  getmultimems                   records max(4096, m / 16), members max(8192, m / 2), listed runs n / 64 + 1024    rv_api.hip, rv_mems.hip
The margin: DBuf::reserve (rv_common.h) allocates bytes + bytes / 8 + 256."""
import numpy as np

MINL = 7
PAIR_TILE, PAIR_SLOTS, PAIR_HDR, PAIR_REC_BYTES = 1024, 16, 1, 16
MULTI_REC_BYTES = 16


def dbuf_bytes(want):
    """what DBuf::reserve allocates for a request below 256 MB"""
    return want + want // 8 + 256


def pair_ovf_cap():
    return dbuf_bytes(4096 * PAIR_REC_BYTES) // PAIR_REC_BYTES


def pair_out_cap(m):
    return dbuf_bytes(PAIR_REC_BYTES * max(4096, m // 64)) // PAIR_REC_BYTES - PAIR_HDR


def first_copy_guess():
    return 4096


def multi_rec_cap(m):
    return dbuf_bytes(MULTI_REC_BYTES * max(4096, m // 32)) // MULTI_REC_BYTES


def multi_mem_cap(m):
    return dbuf_bytes(2 * max(8192, m // 8)) // 2


def multi_cand_cap(m):
    return max(65536, m // 64)


def mems_caps(n):
    return max(4096, n // 16), max(8192, n // 2), n // 64 + 1024


def _text(g, n):
    return "".join("ACGT"[x] for x in g.integers(0, 4, n))


def unrelated_pair(L=30000):
    """two independent uniform texts: at minl 7 thousands of chance MUMs, every tile of the scan beyond its slots"""
    g = np.random.default_rng(3)
    return [_text(g, L), _text(g, L)]


def copies_pair(L=30000):
    """U + Z + U against V + Z + V: every chance match of U and V occurs twice, so the top level has the one MUM through Z and the
    density of unrelated_pair arrives one level down, in two sub-indices"""
    g = np.random.default_rng(5)
    U, V, Z = _text(g, L), _text(g, L), _text(g, 300)
    return [U + Z + U, V + Z + V]


def copies_triple(L=12000):
    """the same shape for three samples"""
    g = np.random.default_rng(7)
    Z = _text(g, 300)
    U, V, W = _text(g, L), _text(g, L), _text(g, L)
    return [U + Z + U, V + Z + V, W + Z + W]


def _snp(g, s, every):
    """a substitution every `every` bases or so (never the same base)"""
    s = list(s)
    p = int(g.integers(0, every))
    while p < len(s):
        s[p] = "ACGT"[("ACGT".index(s[p]) + 1 + int(g.integers(0, 3))) % 4]
        p += 1 + int(g.integers(every // 2, every + every // 2))
    return "".join(s)


def tandem_pair(L=20000, unit=23, copies=60):
    """related samples around a tandem array with its own point mutations in each: repeat witnesses by the hundred"""
    g = np.random.default_rng(11)
    base = _text(g, L)
    arr = _text(g, unit) * copies
    return [base[:L // 2] + _snp(g, arr, 90) + base[L // 2:], _snp(g, base[:L // 2], 100) + _snp(g, arr, 80) + _snp(g, base[L // 2:], 100)]


def repetitive_triple(L=6000, unit=31, copies=120):
    """three samples that are mostly one tandem array, between unique flanks that anchor them: a thousand and more repeat witnesses, and -- the
    suffixes of one phase of the array share ever longer prefixes, copy after copy -- runs of the LCP array that nest deeper than the stack a
    thread of the multi-MEM scan keeps (24 entries), which that scan lists for its wavefront machine"""
    g = np.random.default_rng(13)
    left, right = _text(g, L // 2), _text(g, L // 2)
    arr = _text(g, unit) * copies
    return [_snp(g, left, 150) + _snp(g, arr, 70 + 10 * k) + _snp(g, right, 150) for k in range(3)]


def contig_pair(L=20000):
    """a related pair with two contigs per sample (the second sample's in the other order)"""
    g = np.random.default_rng(19)
    a = _text(g, L)
    b = _snp(g, a, 100)
    return [[a[:L // 2], a[L // 2:]], [b[L // 2:], b[:L // 2]]]
