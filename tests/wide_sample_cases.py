"""inputs of the multi-sample tests at 6 .. 258 samples (tests/test_cpu_wide_sample_cases.py checks the generator itself,
tests/test_gpu_wide_samples.py and tools/fuzz.py --wide use it): one family per sample count k on either side of every place where the
ordinary multi-sample path switches on the NUMBER OF SAMPLES (DESIGN.md section 5 has the table), built on the "variant sites" model of
many_wide_cases.py -- a per-member mutation rate leaves a family of 64 and more members without a single match on every sample.

    one random ancestor of L bases with a tandem array (unit of 3 / 7 / 23 bases, about 120 bases), a repeat of 40 bases in three copies and
      a run of 9 N; the three copies differ in their centre base, and two members carry another copy's centre base (see `family`);
    a variant site every 22 .. 90 bases, each substituted (one other base) in a random non-empty proper subset of the members;
    six regions, each deleted in a subset of the members of 1, k/3, k/2, k-2, k-9 and k-16 members (clamped to 1 .. k-2): the recursion
      meets sub-indices of 2 .. k samples, and lanes whose ranks straddle sub-indices of differing sample counts; samples 15, 16, 31 and 32
      are among the 16 that keep the last region (condition (i));
    an insertion of 60 bases shared by k/4 members;
    an insertion of 44 bases shared by two members, in the middle of 28 bases without a variant site: 13 + 1 + 16 + 1 + 13 with either single
      base private to one of them -- a sub-index of two samples whose pick leaves two children of 28 ranks side by side, each with a pick of
      its own: two sub-indices with a candidate in one tile of a level, which is what overflows the picker's candidate list at one entry per
      region whatever k is (condition (h));
    the last member is the first one again.

Deterministic (random.Random(seed * 1000 + k)), nothing is stored.  SEEDS pins, per k, the first seed at which the oracle alone
(helpers.oracle: construct, getmultimums, align_bench with a trace) finds what the GPU tests are there to meet -- conditions (a) .. (i) of
`missing`; `python tests/wide_sample_cases.py` searches the seeds again and prints the table."""
import collections
import functools
import random

import numpy as np

from helpers import assemble, csr_tuples, oracle

K = (6, 9, 15, 16, 17, 32, 33, 40, 64, 65, 100, 129, 254, 255, 256, 257, 258)
MINL = 12                     # minlength of the recursion and of the first getmultimums list
MINL_FULL = 4                 # ... of the second one, with minn = k
SITE_GAP = (22, 90)
UNITS = (3, 7, 23)
ARRAY, REPEAT, NRUN, INSERT, REGIONS = 120, 40, 9, 60, 6
PRIVATE = (13, 16, 13)
NEIGHBOURS = (15, 16, 31, 32)
SEEDS = {}                    # k -> seed; filled in below


def length(k):
    """bases of the ancestor: about 30 000 / k, at least 300 (the switches depend on k, not on the size: the largest index has about
    70 000 ranks.  600 bases from k = 200 on, about 135 000 ranks, made every recursion of 255 samples and more take 11 .. 16 s)"""
    return max(300, 30000 // k)


def rnd(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def ancestor(rng, L):
    base = list(rnd(rng, L))

    def put(at, s):
        base[at:at + len(s)] = list(s)[:max(0, L - at)]
    unit = rnd(rng, rng.choice(UNITS))
    put(L // 5, unit * (ARRAY // len(unit)))
    rep = rnd(rng, REPEAT)
    marks = rng.sample("ACGT", 3)                  # the copies differ in their centre base
    copies = (L // 3, L // 2 + 17, (4 * L) // 5)
    for at, c in zip(copies, marks):
        put(at, rep[:REPEAT // 2] + c + rep[REPEAT // 2 + 1:])
    put((2 * L) // 3, "N" * NRUN)
    return "".join(base), [at + REPEAT // 2 for at in copies], marks


def family(k, seed, L=None):
    """-> the k members (strings)"""
    L = length(k) if L is None else L
    rng = random.Random(seed * 1000 + k)
    base, centre, marks = ancestor(rng, L)
    fam = [list(base) for _ in range(k)]
    W = L // (2 * REGIONS)
    private_at = 10 * W + W // 4                   # between the fifth and the sixth region; no variant site within 14 bases of it
    at = rng.randint(5, SITE_GAP[0] * 2)
    while at < L:
        if base[at] != "N" and abs(at - private_at) > 14:
            alt = rng.choice([c for c in "ACGT" if c != base[at]])
            for i in rng.sample(range(k), rng.randint(1, k - 1)):
                fam[i][at] = alt
        at += rng.randint(*SITE_GAP)
    # one member carries the first copy's centre base in its second copy as well, another one the second copy's in its first: the words round
    # either centre then occur k times, twice in one sample (condition (g): what a census of the samples is there to refuse)
    i, j = rng.sample(range(1, k - 1), 2)
    fam[j][centre[1]] = marks[0]
    fam[i][centre[0]] = marks[1]
    # what is cut out of / put into each member, as (position in the ancestor, bases removed, text inserted); applied from the right
    edits = [[] for _ in range(k)]
    for r, size in enumerate((1, k // 3, k // 2, k - 2, k - 9, k - 16)):
        # (the last region: the samples on either side of the sixteenth separator and of the census' word boundary stay among the 16 that keep it)
        pool = [i for i in range(k) if r < REGIONS - 1 or k < 17 or i not in NEIGHBOURS]
        size = max(1, min(k - 2, size))
        for i in rng.sample(pool if len(pool) >= size else range(k), size):
            edits[i].append(((2 * r + 1) * W, W // 2, ""))
    ins = rnd(rng, INSERT)
    for i in rng.sample(range(k), max(2, k // 4)):
        edits[i].append((L // 2 + 5, 0, ins))
    p, q = rng.sample(range(1, k - 1), 2)
    left, mid, right, x, y = rnd(rng, PRIVATE[0]), rnd(rng, PRIVATE[1]), rnd(rng, PRIVATE[2]), rng.sample("ACGT", 2), rng.sample("ACGT", 2)
    edits[p].append((private_at, 0, left + x[0] + mid + y[0] + right))
    edits[q].append((private_at, 0, left + x[1] + mid + y[1] + right))
    out = []
    for s, ed in zip(fam, edits):
        for at, cut, put in sorted(ed, reverse=True):
            s[at:at + cut] = list(put)
        out.append("".join(s))
    out[-1] = out[0]
    return out


def aset(a):
    """anchors of the oracle (l, n, off, pos) or of the library (l, off, pos) -> sorted [(l, (positions...))]"""
    l, off, pos = (a[0], a[2], a[3]) if len(a) == 4 else a
    return sorted((int(l[j]), tuple(int(x) for x in pos[off[j]:off[j + 1]])) for j in range(len(l)))


def doubled_root_intervals(SA, LCP, SO, k, minl=MINL):
    """condition (g): LCP intervals of exactly k ranks and a value of minl and more at the root (what the picker's census is asked about) in
    which a sample occurs twice.  -> (their number, the number of those whose two ranks of one sample are not neighbours)"""
    n = len(SA)
    lcp = np.asarray(LCP).astype(np.int64)
    if n < k + 1:
        return 0, 0
    inner = np.lib.stride_tricks.sliding_window_view(lcp[1:], k - 1).min(axis=1)      # inner[lb] = min LCP[lb+1 .. lb+k-1]
    nlb = len(inner)                                                                   # lb = 0 .. n - k
    after = np.append(lcp[k:], 0)[:nlb]                                                # LCP[lb + k] (0 past the end)
    cand = np.nonzero((inner >= minl) & (lcp[:nlb] < inner) & (after < inner))[0]
    so = np.asarray(SO)
    twice = apart = 0
    for lb in cand:
        sm = so[np.asarray(SA[lb:lb + k]).astype(np.int64)].astype(np.int64)
        if len(np.unique(sm)) < k:
            twice += 1
            first = {}
            for r, s in enumerate(sm):
                if s in first and r - first[s] > 1:
                    apart += 1
                    break
                first.setdefault(int(s), r)
    return twice, apart


@functools.lru_cache(maxsize=None)
def reference(k, seed, sa64=False, L=None):
    """everything the oracle says about one family, computed once: arrays of the root, both getmultimums lists, the recursion's trace,
    anchors, text and counters, and the figures of conditions (a) .. (i)"""
    seqs = family(k, seed, L)
    T, nsep, nodes = assemble(seqs)
    O = oracle(sa64)
    c = O.construct(T, nsep, k)
    SA, LCP = c["SA"].copy(), c["LCP"].copy()
    mums = csr_tuples(*O.getmultimums(c["tbuf"], c["SA"], c["LCP"], c["SO"], nsep, k, MINL, 2))
    mums_full = csr_tuples(*O.getmultimums(c["tbuf"], c["SA"], c["LCP"], c["SO"], nsep, k, MINL_FULL, k))
    twice, apart = doubled_root_intervals(SA, LCP, c["SO"], k)
    r = O.align_bench(c, nodes, MINL, 2, trace_cap=4 * len(T) // MINL + 1000)      # (splits the arrays of c in place)
    tr = r["trace"]
    l, n, off, pos = r["anchors"]
    seps = np.asarray(nsep, dtype=np.int64)
    small_high = small_15_16 = small_31_32 = 0
    for j in range(len(l)):
        ps = np.asarray(pos[off[j]:off[j + 1]], dtype=np.int64)
        if len(ps) <= 16:
            sm = set(int(x) for x in np.searchsorted(seps, ps, side="left"))
            small_high += max(sm) >= 32
            small_15_16 += {15, 16} <= sm
            small_31_32 += {31, 32} <= sm
    ns, picked = tr["nsamples"].astype(np.int64), tr["picked"].astype(bool)
    bands = collections.OrderedDict((name, (int(((ns >= lo) & (ns <= hi)).sum()), int(((ns >= lo) & (ns <= hi) & picked).sum())))
                                    for name, lo, hi in (("le16", 0, 16), ("17_32", 17, 32), ("33_64", 33, 64), ("gt64", 65, 1 << 30), ("ge17", 17, 1 << 30), ("ge255", 255, 1 << 30)))
    pairs = 0      # (h): picked sub-indices of two samples and at most 64 ranks that have another one at their depth
    small = picked & (ns == 2) & (tr["n"].astype(np.int64) <= 64)
    for d in np.unique(tr["depth"][small]):
        pairs += int((small & (tr["depth"] == d)).sum()) // 2
    figs = dict(k=k, small_pairs=pairs, small_15_16=small_15_16, small_31_32=small_31_32, seed=seed, first_len=len(seqs[0]), ranks=len(T), subs=len(tr), picked=int(picked.sum()), anchors=len(l),
                subset_anchors=int((np.asarray(n) < k).sum()), mums_full_n=sum(1 for m in mums if m[1] == k), mums_subset_n=sum(1 for m in mums if m[1] < k),
                small_high=small_high, bands=bands, doubled=twice, doubled_apart=apart)
    assert int(r["stats"]["anchored_bp"]) == int(np.asarray(l, dtype=np.int64).sum())
    return dict(seqs=seqs, T=T, nsep=nsep, SA=SA, LCP=LCP, mums=mums, mums_full=mums_full, run=r, trace=tr, anchors=aset(r["anchors"]), text=r["T"],
                splits=int(r["stats"]["nsplits"]), steps=int(r["stats"]["nsteps"]), anchored_bp=int(r["stats"]["anchored_bp"]), figs=figs)


def missing(figs):
    """the conditions a pinned family has to meet, from the oracle's figures alone -> the letters of those it misses"""
    k, b, out = figs["k"], figs["bands"], []
    if figs["anchors"] < 8:
        out.append("a")
    if figs["subset_anchors"] < 1 or figs["mums_full_n"] < 1 or figs["mums_subset_n"] < 1:
        out.append("b")
    if k >= 17 and (b["le16"][1] < 1 or b["ge17"][1] < 1):      # (picked in a band implies visited)
        out.append("c")
    if k >= 33 and figs["small_high"] < 1:
        out.append("d")
    if k >= 65 and (b["le16"][1] < 1 or b["gt64"][1] < 1):
        out.append("e")
    if k >= 255 and b["ge255"][1] < 1:
        out.append("f")
    if figs["doubled_apart"] < 1:      # (asked for: two ranks of one sample that are not neighbours, so that a census of neighbours would not do)
        out.append("g")
    if figs["small_pairs"] < 1:
        out.append("h")
    if (k >= 17 and figs["small_15_16"] < 1) or (k >= 33 and figs["small_31_32"] < 1):
        out.append("i")
    return out


def search(k, most=50):
    """the first seed of 1 .. most whose family meets every condition"""
    for seed in range(1, most + 1):
        if not missing(reference(k, seed)["figs"]):
            return seed
    return None


SEEDS.update({6: 1, 9: 1, 15: 1, 16: 1, 17: 1, 32: 1, 33: 2, 40: 1, 64: 1, 65: 17, 100: 7, 129: 3, 254: 2, 255: 2, 256: 3, 257: 1, 258: 7})


if __name__ == "__main__":
    for k in K:
        s = search(k)
        f = reference(k, s)["figs"] if s else None
        print(k, s, f and {x: (dict(v) if x == "bands" else v) for x, v in f.items()}, flush=True)
