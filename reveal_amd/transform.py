"""The first stage of `reveal transform` (reveal/transform.py:252-293): MUMs of a reference against the contigs of a draft assembly, forward
and reverse-complemented, tagged with the sequences they lie in (addctginfo) and merged along their diagonals (clustermumsbydiagonal) into the
`blocks` list that glocalchain, extendblocks and the breakpoint graph go on with.

    synteny_blocks(reference, contigs)      the whole stage through index.getblocks: the MUMs never leave device memory
    blocks_python / blocks_native / blocks_device      the rule on a list of MUMs: plain Python, host C++ (rv_blocks_host), the kernels (rv_blocks_records)

The rule is stated once in include/reveal_amd.h (rv_getblocks).  One departure from the reference: an empty MUM list gives an empty block list (its
forward leg raises IndexError on mums[0]).  A sequence id for a position behind every range is the number of ranges.  Not done here: glocalchain and
everything behind it, --cutn, a reverse complement made on the device, a form for many inputs at once.
"""
from bisect import bisect_left

import numpy as np

from . import _lib
from .reveallib import error

__all__ = ["blocks_python", "blocks_native", "blocks_device", "synteny_blocks", "error"]


def _records(mums):
    """[(l, (a, b), ...)] -> l (uint32), a, b (int64)"""
    n = len(mums)
    l = np.fromiter((m[0] for m in mums), dtype=np.uint32, count=n)
    a = np.fromiter((m[1][0] for m in mums), dtype=np.int64, count=n)
    b = np.fromiter((m[1][1] for m in mums), dtype=np.int64, count=n)
    return l, a, b


def _ends(ranges):
    return np.ascontiguousarray(np.array([int(e) for _, e in ranges], dtype=np.int64))


def _tuples(o, cols):
    return [(s1, e1, s2, e2, o, sc, rf, cg) for s1, e1, s2, e2, sc, rf, cg in zip(*[c.tolist() for c in cols])]


def blocks_python(mums, ranges, cluster=True, maxdist=30, minclustsize=50, rcmums=False):
    """addctginfo + clustermumsbydiagonal restated: mums = [(l, (a, b), ...)] as getmums gives them, ranges = [(begin, end)] of every sequence in
    order of addition -> [(s1, e1, s2, e2, o, score, refid, ctgid)]"""
    ends = [int(e) for _, e in ranges]
    o = 1 if rcmums else 0
    recs = [(int(m[0]), int(m[1][0]), int(m[1][1])) for m in mums]
    recs = [(l, a, b, bisect_left(ends, a), bisect_left(ends, b)) for l, a, b in recs]      # ids: how many sequences end in front of the position
    recs.sort(key=lambda r: (r[2], r[1]))                                                   # by reference position, then (stably) by query position
    if not cluster:
        return [(a, a + l, b, b + l, o, l, rid, cid) for l, a, b, rid, cid in recs]
    if rcmums:
        first = lambda r: r[1] + r[2] + r[0]
        recs.sort(key=lambda r: (first(r), r[1] - (r[2] + r[0])))
    else:
        first = lambda r: r[1] - r[2]
        recs.sort(key=lambda r: (first(r), r[1] + r[2]))
    out = []
    cur = prev = None                   # the running cluster [first member, last member, score], the previous record
    for r in recs:
        if prev is not None and first(r) == first(prev) and r[3:] == prev[3:]:
            dist = r[1] - (prev[1] + prev[0])
            if dist < 0:
                raise error("blocks: overlapping matches on a diagonal")
            if dist < maxdist:
                cur[1] = r
                cur[2] += r[0]
                prev = r
                continue
        if cur is not None:
            out.append(cur)
        cur = [r, r, r[0]]
        prev = r
    if cur is not None:
        out.append(cur)
    blocks = []
    for F, L, score in out:
        if score < minclustsize:
            continue
        if rcmums:
            blocks.append((F[1], L[1] + L[0], L[2], F[2] + F[0], o, score, F[3], F[4]))
        else:
            blocks.append((F[1], L[1] + L[0], F[2], L[2] + L[0], o, score, F[3], F[4]))
    return blocks


def blocks_native(mums, ranges, cluster=True, maxdist=30, minclustsize=50, rcmums=False, sa64=False):
    """the same through the library's host C++ (rv_blocks_host): no device is asked for"""
    lib = _lib.get(sa64)
    l, a, b = _records(mums)
    ends = _ends(ranges)
    n = len(l)
    cols = [np.zeros(max(n, 1), dtype=np.int64) for _ in range(5)] + [np.zeros(max(n, 1), dtype=np.int32) for _ in range(2)]
    counts = np.zeros(2, dtype=np.int64)
    k = lib.dll.rv_blocks_host(n, l.ctypes.data, a.ctypes.data, b.ctypes.data, 1 if rcmums else 0, len(ends), ends.ctypes.data, 1 if cluster else 0,
                               int(maxdist), int(minclustsize), counts.ctypes.data, *[c.ctypes.data for c in cols], max(n, 1))
    if k < 0:
        raise error(lib.err())
    return _tuples(1 if rcmums else 0, [c[:k] for c in cols])


def blocks_device(mums, ranges, cluster=True, maxdist=30, minclustsize=50, rcmums=False, sa64=False, index=None):
    """the same through the kernels of getblocks (rv_blocks_records).  index: a handle that lends its stream and workspace (constructed or not);
    without one a fresh index object is made for the call"""
    if index is None:
        from . import reveallib, reveallib64
        index = (reveallib64 if sa64 else reveallib).index()
    lib = index._lib
    l, a, b = _records(mums)
    ends = _ends(ranges)
    k = lib.dll.rv_blocks_records(index._h, len(l), l.ctypes.data, a.ctypes.data, b.ctypes.data, 1 if rcmums else 0, len(ends), ends.ctypes.data,
                                  1 if cluster else 0, int(maxdist), int(minclustsize))
    if k < 0:
        raise error(lib.err())
    r = index._fetch_blocks(k)
    return _tuples(1 if rcmums else 0, [r[c] for c in ("s1", "e1", "s2", "e2", "score", "refid", "ctgid")])


def _sequences(src):
    """a FASTA path, or a list of sequences / (name, sequence) pairs -> [(name, sequence)]"""
    if isinstance(src, str):
        from .rem import fasta_reader
        return list(fasta_reader(src))
    out = []
    for k, s in enumerate(src):
        name, seq = s if isinstance(s, tuple) else ("seq%d" % k, s)
        out.append((name, seq))
    return out


def synteny_blocks(reference, contigs, minlength=20, cluster=True, maxdist=30, mincluster=50, minctglength=10000, sa64=False):
    """transform.py:228-293: reference and contigs (FASTA paths, or lists of sequences) -> dict(blocks, ctg2range, sep, rlength, qlength, mums), what
    glocalchain is handed.  Sequences shorter than minctglength are skipped in both inputs (transform.py:241).  Sample 0 is the reference, sample 1 the
    contigs; blocks = the forward blocks (construct(rc=0), getblocks) followed by the reverse-complement ones (construct(rc=1), getblocks); mums =
    (forward, reverse-complement) MUM counts; also refnames / ctgnames of the sequences kept."""
    from . import reveallib, reveallib64
    idx = (reveallib64 if sa64 else reveallib).index()
    ctg2range, names = [], ([], [])
    for k, src in enumerate((reference, contigs)):
        idx.addsample("reference" if k == 0 else "contigs")
        for name, seq in _sequences(src):
            if len(seq) < minctglength:
                continue
            ctg2range.append(idx.addsequence(seq))
            names[k].append(name)
    if not names[0] or not names[1]:
        raise error("synteny_blocks: no sequence of at least minctglength in %s" % ("the reference" if not names[0] else "the contigs"))
    idx.construct(rc=0)
    fwd = idx.getblocks_arrays(minlength, cluster, maxdist, mincluster)
    idx.construct(rc=1)
    rc = idx.getblocks_arrays(minlength, cluster, maxdist, mincluster)
    sep, n = idx.nsep[0], idx.n
    keys = ("s1", "e1", "s2", "e2", "score", "refid", "ctgid")
    blocks = _tuples(0, [fwd[c] for c in keys]) + _tuples(1, [rc[c] for c in keys])
    return dict(blocks=blocks, ctg2range=ctg2range, sep=sep, rlength=sep, qlength=n - sep, mums=(fwd["info"]["mums"], rc["info"]["mums"]),
                refnames=names[0], ctgnames=names[1])
