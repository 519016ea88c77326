"""inputs of the align_many tests with the reference's default picker on jobs of three and more sequences (RV_MANY_CHAIN_MULTI;
tests/test_cpu_many_chain_multi.py checks the list and the golden file, tests/test_gpu_many_chain_multi.py runs it): the class jobs of
many_multi_cases, a class of its own whose members carry a swapped, dropped or duplicated block shared by a random subset of them, the corner jobs of
the shared launches, and constructed jobs for what only this picker does on several samples -- a `rest` child that anchors, the tie of `segment`,
children down to two live samples, tandem arrays.  Deterministic.  The expected results (tests/golden/many_chain_multi.json, written by
tools/gen_many_chain_multi_golden.py) come from `rem.align` on the REFERENCE's own index module."""
import json
import os
import random

import many_cases as mc
import many_chain_cases as cc
import many_multi_cases as mm

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "many_chain_multi.json")

# (name, keyword arguments of rem.align); what is not named: wpen 1, wscore 1, sumofpairs, trim, seedsize 10000, maxmums 10000, minn 2
SETS = (
    ("default", dict(minlength=20)),
    ("wpen4", dict(minlength=20, wpen=4)),
    ("wscore3", dict(minlength=20, wscore=3)),
    ("star-avg", dict(minlength=20, gcmodel="star-avg")),
    ("star-med", dict(minlength=20, gcmodel="star-med")),
    ("minl10", dict(minlength=10)),
    ("minl1", dict(minlength=1)),
    ("minn3", dict(minlength=20, minn=3)),
)
PER_CLASS = 5            # one job per k of many_multi_cases.K_VALUES and class
N_REARRANGED = 40
CORNERS = ("three_single_bases", "sixteen_single_bases", "ranks_512", "ranks_513", "ranks_2048", "k16_full")


def rearranged(rng, k):
    """k members of a family of blocks; a random proper subset of them carries the same rearrangement: two blocks swapped, maybe one dropped, maybe
    one repeated behind the end"""
    nb = rng.randint(3, 6)
    top = max(24, (mm.MAX_RANKS - k) // k // (nb + 1) - 8)
    blocks = [mc.rnd(rng, rng.randint(22, min(90, top))) for _ in range(nb)]
    order = list(range(nb)); i, j = rng.sample(range(nb), 2); order[i], order[j] = order[j], order[i]
    if rng.random() < 0.5: order.pop(rng.randrange(len(order)))
    tail = (mc.rnd(rng, rng.randint(1, 20)), rng.randrange(nb)) if rng.random() < 0.5 else None
    sub = set(rng.sample(range(k), rng.randint(1, k - 1)))
    out = []
    for s in range(k):
        o = order if s in sub else range(nb)
        t = "".join(mc.mutate(rng, blocks[b], 0.01) for b in o)
        if s in sub and tail: t += tail[0] + blocks[tail[1]]
        out.append(t)
    return out


def constructed():
    rng = random.Random(81)
    x, y = mc.rnd(rng, 90), mc.rnd(rng, 70)
    e1, e2 = mc.rnd(rng, 60), mc.rnd(rng, 60)
    fam = [mc.mutate(rng, mc.rnd(random.Random(82), 200), 0.01) for _ in range(4)]
    a, b, c = mc.rnd(rng, 50), mc.rnd(rng, 40), mc.rnd(rng, 50)
    u3, u4 = mc.rnd(rng, 3), mc.rnd(rng, 5)
    l3, r3, l4, r4 = (mc.rnd(rng, 30) for _ in range(4))
    return [
        # {0, 1} and {2, 3} are two unrelated pairs: `segment` takes the pair with the larger z, the rest child of two samples anchors itself
        ("two_pairs", [x, mc.mutate(rng, x, 0.02), y, mc.mutate(rng, y, 0.02)]),
        # ... with equal z for both groups (one match of 60 bases each): the tie of `segment` goes to the group seen first
        ("two_pairs_tie", [e1, e1, e2, e2]),
        ("two_pairs_tie_interleaved", [e1, e2, e1, e2]),
        ("five_one_unrelated", fam[:2] + [mc.rnd(rng, 150)] + fam[2:]),
        # the third sample is a piece of the middle: the children of its anchor go on with two live samples
        ("down_to_two", [a + b + c, mc.mutate(rng, a, 0.03) + b + mc.mutate(rng, c, 0.03), b]),
        # tandem arrays with other copy numbers per member: overlapping matches, trimmed on more than one coordinate
        ("tandem3", [l3 + u3 * n + r3 for n in (9, 12, 10)]),
        ("tandem4", [l4 + u4 * n + r4 for n in (6, 8, 7, 8)]),
        ("tandem_mixed", [l3 + u3 * 10 + r3 + u4 * 5 + r4, l3 + u3 * 12 + r3 + u4 * 7 + r4, l3 + u3 * 9 + r3 + u4 * 6 + r4]),
    ]


def jobs():
    """-> [(class, [seq, ..])]: many_multi_cases.class_jobs(PER_CLASS), N_REARRANGED `rearranged` jobs (k cycling 3, 4, 5, 8, 16), the corner jobs the
    shared launches take, the constructed jobs"""
    def fit(fam):                                   # (a family of sixteen can come out above 2048 ranks: every member cut to an equal share)
        return [s[:(mm.MAX_RANKS - len(fam)) // len(fam)] for s in fam] if mm.ranks(fam) > mm.MAX_RANKS else list(fam)
    out = [(cls, fit(fam)) for cls, k, fam in mm.class_jobs(PER_CLASS)]
    rng = random.Random(79)
    out += [("rearranged", fit(rearranged(rng, mm.K_VALUES[j % len(mm.K_VALUES)]))) for j in range(N_REARRANGED)]
    corners = {name: fam for name, fam, _ in mm.corner_jobs()}
    out += [("corner:" + name, list(corners[name])) for name in CORNERS]
    return out + [("made:" + name, fam) for name, fam in constructed()]


def picker_args(kw):
    return cc.picker_args(kw)


def run_kw(kw):
    """keyword arguments of align_many for a set: minlength and minn of the run"""
    return dict(minlength=kw["minlength"], minn=kw.get("minn", 2))


def rem_align_job(seqs, indexmod=None, **kw):
    """`rem.align` on ONE job -> (sorted anchors [(l, (pos, ..) in the order graphalign got them)], final text)"""
    return cc.rem_align_job(seqs, indexmod=indexmod, **kw)


sha = cc.sha


def load_golden():
    """-> {set name: [(sorted anchors [(l, (members in emitted order))], sha256 of the final text)] in the order of jobs()}"""
    with open(GOLDEN) as f:
        doc = json.load(f)
    assert doc["sets"] == [n for n, _ in SETS] and doc["jobs"] == len(jobs())
    return {n: [([(a[0], tuple(a[1:])) for a in r["anchors"]], r["sha"]) for r in doc["results"][n]] for n, _ in SETS}


def sample_sets(seqs, anchors):
    """the sample of every member of every anchor -> [frozenset of samples]"""
    ends, at = [], 0
    for s in seqs:
        at += len(s) + 1
        ends.append(at)
    return [frozenset(next(q for q, e in enumerate(ends) if p < e) for p in pos) for _, pos in anchors]


def kernel_scan(T, SA, LCP, nsamples, minl, minn=2):
    """the scan of k_leaf_multi_chain (csrc/rv_leaf_multi_chain.hip) restated on the ROOT index of a job: a lane owns an upper rank u and walks the
    windows [u - n + 1, u], n = 2 .. nsamples; lanes by ascending u -> [(l, (member positions in rank order))] in the order the kernel lists them"""
    n, out = len(SA), []
    ends = [i for i, c in enumerate(T) if c == ord("$")]
    smp = lambda p: next(q for q, e in enumerate(ends) if p <= e)
    bwt = lambda r: T[SA[r] - 1] if SA[r] > 0 else ord("$")
    special = lambda c: c in (ord("N"), ord("$")) or ord("a") <= c <= ord("z")
    need = max(minl, 1)
    for u in range(1, n):
        nxt = LCP[u + 1] if u + 1 < n else 0
        if T[SA[u]] == ord("$"):
            continue
        seen, l, cnext, lm = {smp(SA[u])}, None, bwt(u), False
        for k in range(2, nsamples + 1):
            r = u - k + 1
            if r < 0:
                break
            l = LCP[r + 1] if l is None else min(l, LCP[r + 1])
            if l < need or l <= nxt:
                break
            s = smp(SA[r])
            if T[SA[r]] == ord("$") or s in seen:
                break
            seen.add(s)
            c = bwt(r)
            lm = lm or c != cnext or special(c)
            cnext = c
            if k >= max(minn, 2) and lm and (r == 0 or LCP[r] < l):
                out.append((int(l), tuple(int(SA[q]) for q in range(r, u + 1))))
    return out
