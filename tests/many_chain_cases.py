"""inputs of the align_many tests with the reference's default picker (tests/test_cpu_many_chain.py checks the list and the golden file,
tests/test_gpu_many_chain.py runs it): the class jobs of many_cases, a class of its own whose alleles carry a swapped, dropped or duplicated block --
where trimming and chaining choose other anchors than the longest match -- and two jobs of exactly 2048 ranks.  Deterministic.  The expected results
(tests/golden/many_chain.json, written by tools/gen_many_chain_golden.py) come from `rem.align` on the REFERENCE's own index module."""
import hashlib
import json
import os
import random

import many_cases as mc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "many_chain.json")

# (name, keyword arguments of rem.align); what is not named: wpen 1, wscore 1, sumofpairs, trim, seedsize 10000, maxmums 10000
SETS = (
    ("default", dict(minlength=20)),
    ("wpen4", dict(minlength=20, wpen=4)),
    ("wscore3", dict(minlength=20, wscore=3)),
    ("star-avg", dict(minlength=20, gcmodel="star-avg")),
    ("star-med", dict(minlength=20, gcmodel="star-med")),
    ("minl10", dict(minlength=10)),
    ("minl1", dict(minlength=1)),         # the most candidates per sub-index: the corner of list capacity and chain length
)
N_CLASS = 44
N_REARRANGED = 60


def rearranged(rng):
    nb = rng.randint(3, 8)
    blocks = [mc.rnd(rng, rng.randint(22, 120)) for _ in range(nb)]
    order = list(range(nb)); i, j = rng.sample(range(nb), 2); order[i], order[j] = order[j], order[i]
    if rng.random() < 0.5: order.pop(rng.randrange(len(order)))
    a = "".join(blocks); b = "".join(mc.mutate(rng, blocks[k], 0.01) for k in order)
    if rng.random() < 0.5:
        k = rng.randrange(nb); b = b + mc.rnd(rng, rng.randint(1, 30)) + blocks[k]
    return a, b


def full_jobs():
    """two jobs of exactly 2048 ranks: unrelated sequences; a sequence against itself with one substitution every 21 bases"""
    rng = random.Random(78)
    a, b = mc.rnd(rng, 1023), mc.rnd(rng, 1023)
    s = mc.rnd(rng, 1023)
    t = list(s)
    for i in range(10, len(t), 21):
        t[i] = "ACGT"[("ACGT".index(t[i]) + 1) % 4]
    return [("full-unrelated", (a, b)), ("full-periodic", (s, "".join(t)))]


def jobs():
    """-> [(class, (a, b))]: many_cases.class_jobs(4), 60 `rearranged` jobs, the two jobs of 2048 ranks"""
    out = list(mc.class_jobs(4))
    rng = random.Random(77)
    out += [("rearranged", rearranged(rng)) for _ in range(N_REARRANGED)]
    return out + full_jobs()


def picker_args(kw):
    """the schemes.PickerArgs `rem.align(.., **kw)` builds (reveal_amd/rem.py align)"""
    from reveal_amd import schemes
    return schemes.PickerArgs(wscore=kw.get("wscore", 1), wpen=kw.get("wpen", 1), maxmums=kw.get("maxmums", 10000), seedsize=kw.get("seedsize", 10000),
                              gcmodel=kw.get("gcmodel", "sumofpairs"), trim=kw.get("trim", True), pcutoff=kw.get("pcutoff", 1e-8))


def rem_align_job(seqs, indexmod=None, **kw):
    """`rem.align` on ONE job, as `reveal refine` calls it for a bubble, the anchors recorded through a wrapped graphalign (the way
    tests/test_cpu_graph_native.py run_and_record does) -> (sorted anchors [(l, (pos, ..))], final text)"""
    from reveal_amd import rem
    rec = []

    class Rec(rem.GraphAligner):
        def graphalign(self, index, mum):
            rec.append((int(mum[0]), tuple(int(p) for _, p in mum[2])))
            return super().graphalign(index, mum)
    orig = rem.GraphAligner
    rem.GraphAligner = Rec
    try:
        G, idx = rem.align([("s%d" % k, s) for k, s in enumerate(seqs)], indexmod=indexmod, **kw)
    finally:
        rem.GraphAligner = orig
    T = idx.T
    return sorted(rec), (T if isinstance(T, str) else T.decode("latin-1"))


def sha(text):
    return hashlib.sha256(text.encode("latin-1") if isinstance(text, str) else bytes(text)).hexdigest()


def load_golden():
    """-> {set name: [(sorted anchors [(l, (pa, pb))], sha256 of the final text)] in the order of jobs()}"""
    with open(GOLDEN) as f:
        doc = json.load(f)
    assert doc["sets"] == [n for n, _ in SETS] and doc["jobs"] == len(jobs())
    return {n: [([(a[0], (a[1], a[2])) for a in r["anchors"]], r["sha"]) for r in doc["results"][n]] for n, _ in SETS}
