"""The first stage of `reveal transform` (reveal/transform.py:252-293): MUMs of a reference against the contigs of a draft assembly, forward
and reverse-complemented, tagged with the sequences they lie in (addctginfo) and merged along their diagonals (clustermumsbydiagonal) into the
`blocks` list that glocalchain, extendblocks and the breakpoint graph go on with.

    synteny_blocks(reference, contigs)      the whole stage through index.getblocks: the MUMs never leave device memory
    blocks_python / blocks_native / blocks_device      the rule on a list of MUMs: plain Python, host C++ (rv_blocks_host), the kernels (rv_blocks_records)

The rule is stated once in include/reveal_amd.h (rv_getblocks).  One departure from the reference: an empty MUM list gives an empty block list (its
forward leg raises IndexError on mums[0]).  A sequence id for a position behind every range is the number of ranges.

The second stage (transform.py:301-360, 947-1180): glocalchain, run on the reference axis until a pass drops nothing and then on the query axis.

    synteny_chain(reference, contigs)       synteny_blocks + glocal_filter: what merge_consecutive is handed at transform.py:377
    glocal_filter(blocks, ...)              both fixed-point loops in one call (rv_glocal_filter); info says which route ran
    glocalchain_python / glocalchain_native / glocalchain_device      one pass: plain Python, host C++ (rv_glocal_host), the kernels (rv_glocal_blocks)

That rule is stated in include/reveal_amd.h as well (rv_glocal_filter).  The library's arithmetic is 64-bit integer: it takes non-negative integral
weights (2.0 counts as 2) whose largest possible score stays inside 62 bits (rv_glocal_admit); anything else takes glocalchain_python, which uses
Python's own arithmetic.  Departures: every list entry is a block of its own (the reference's dictionary merges equal tuples), an empty list gives
an empty chain.

The third stage and the chain's tail (transform.py:376-435, 528-530, 713-935, 1334-1485): merge_consecutive, overlap removal, the optimise loop,
chainscore, extendblocks.

    synteny_layout(reference, contigs)      everything above and below in one call, the block list in columns until merge_consecutive has made it small
    merge_consecutive_python / merge_consecutive_native / merge_consecutive_device, merge_arrays      the merge: plain Python, host C++ (rv_merge_host), the
                                            kernels (rv_merge_blocks); merge_arrays takes columns and the filter's chain as `sel`
    chain_tail(chain, ...)                  what follows glocal_filter, on tuples -> the chain the bed file reads, its weight, cost and edge costs, the extended list
    remove_overlap_python, chainscore_python / chainscore_native, optimise_python / optimise_native, optimise_loop, extendblocks_python      its stages

The merge rule and the rules of chainscore and optimise are stated in include/reveal_amd.h (rv_merge_blocks, rv_chainscore_host).  Where the reference
raises (the pop loop of remove_overlap_* emptying its list, an assert), transform.error is raised.  None of these functions changes its argument (the
reference's sort and rebuild theirs in place).

Not done here: the bed file and the breakpoint graph; useheap; non-integral weights outside Python; the chain handed from the filter to the merge in
device memory (it crosses as `sel`); the getblocks output kept in device memory across construct(rc=1); --cutn; a form for many inputs at once.
"""
from bisect import bisect_left

import numpy as np

from . import _lib
from .reveallib import error

__all__ = ["blocks_python", "blocks_native", "blocks_device", "synteny_blocks", "glocalchain_python", "glocalchain_native", "glocalchain_device",
           "glocal_filter", "glocal_arrays", "glocal_admit", "synteny_chain", "merge_consecutive_python", "merge_consecutive_native",
           "merge_consecutive_device", "merge_arrays", "remove_overlap_python", "chainscore_python", "chainscore_native", "optimise_python", "optimise_native",
           "optimise_loop", "extendblocks_python", "chain_tail", "synteny_layout", "error"]


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
    (forward, reverse-complement) MUM counts; also refnames / ctgnames of the sequences kept, and text = index.text_info() behind the second getblocks (by
    default the text went up once: construct(rc=1) reverses it in device memory)."""
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
    text = idx.text_info()
    sep, n = idx.nsep[0], idx.n
    keys = ("s1", "e1", "s2", "e2", "score", "refid", "ctgid")
    blocks = _tuples(0, [fwd[c] for c in keys]) + _tuples(1, [rc[c] for c in keys])
    return dict(blocks=blocks, ctg2range=ctg2range, sep=sep, rlength=sep, qlength=n - sep, mums=(fwd["info"]["mums"], rc["info"]["mums"]),
                refnames=names[0], ctgnames=names[1], text=text)


# ---- glocalchain (transform.py:947-1180, useheap=False); the rule: include/reveal_amd.h, rv_glocal_filter ---------------------------------------------
_W = ("rearrangecost", "inversioncost", "_lambda", "eps", "alfa", "gapopen")
GLOCAL_DEFAULTS = dict(rearrangecost=1000, inversioncost=1, lastn=50, lastbp=10000, _lambda=5, eps=1, alfa=1, gapopen=10)             # the function's own
TRANSFORM_DEFAULTS = dict(rearrangecost=10000, inversioncost=5, lastn=50, lastbp=20000, _lambda=3, eps=2, alfa=2, gapopen=1)          # the command line's


def _gapcost(b1, b2, w, c1, c2):
    """transform.py:1182-1244 for two blocks inside one reference sequence and one contig, b1 in front of b2 on axis c1"""
    d1 = b2[c1] - b1[c1 + 1]
    if b1[4] == b2[4]:
        fwd = b1[4] == 0
        if (b2[c2] < b1[c2]) if fwd else (b2[c2] > b1[c2]):                  # against the orientation: always a rearrangement
            return w["gapopen"] + w["rearrangecost"] + w["eps"] * (d1 if d1 > 0 else 0)
        d2 = (b2[c2] - b1[c2 + 1]) if fwd else (b1[c2] - b2[c2 + 1])
        inv = 0
    else:
        d1 = max(0, d1)
        d2 = max(0, (b2[c2] - b1[c2 + 1]) if b2[c2] > b1[c2] else (b1[c2] - b2[c2 + 1]))
        inv = w["inversioncost"]
    return w["gapopen"] + min(w["rearrangecost"], w["_lambda"] * abs(d1 - d2)) + w["eps"] * max(min(d1, d2), 0) + inv


def _glocal_cost(p, b, ctg2range, w, axis):
    """what it costs to go from predecessor p to block b (transform.py:1070-1127); a dummy has refid None"""
    c1, c2 = (0, 2) if axis == 0 else (2, 0)
    if p[6] is None and b[6] is None:
        return w["gapopen"] + abs(b[c1] - p[c1 + 1]) * w["eps"]
    if b[6] is None or p[6] is None:                                        # the dummy is made relative to the real block: same sequences, same orientation
        real, dummy = (p, b) if b[6] is None else (b, p)
        x = (real[c2 + 1] if real[4] == 0 else real[c2]) if b[6] is None else (real[c2] if real[4] == 0 else real[c2 + 1])
        rel = [None] * 8
        rel[c1], rel[c1 + 1], rel[c2], rel[c2 + 1], rel[4], rel[5], rel[6], rel[7] = dummy[c1], dummy[c1 + 1], x, x, real[4], 0, real[6], real[7]
        return _gapcost(p, rel, w, c1, c2) if b[6] is None else _gapcost(rel, b, w, c1, c2)
    if p[6] == b[6] and p[7] == b[7]:
        return _gapcost(p, b, w, c1, c2)
    # across contigs or reference sequences without passing a dummy
    if (p[6] == b[6] and axis == 0) or (p[7] == b[7] and axis == 1):
        ps, pe = ctg2range[p[7] if axis == 0 else p[6]]                         # the sequences on the other axis
        bs, be = ctg2range[b[7] if axis == 0 else b[6]]
        cp = abs(pe - p[c2 + 1]) if p[4] == 0 else abs(p[c2] - ps)
        if axis == 0:
            cb = abs(be - b[c2 + 1]) if b[4] == 0 else abs(b[c2] - bs)
        else:
            cb = abs(b[c2] - bs) if b[4] == 0 else abs(be - b[c2 + 1])
        return w["gapopen"] + min(w["rearrangecost"], (cp + cb) * w["eps"])
    return w["rearrangecost"] + w["gapopen"] + abs(b[c1] - p[c1 + 1]) * w["eps"]


def _glocal_dummies(rlength, ctg2range, axis):
    """(start, [dummies]) of an axis (transform.py:951-970): a dummy per sequence end, `start` at the first sequence's begin"""
    start, out = None, []
    if axis == 0:
        for k, (s, e) in enumerate(ctg2range):
            if s >= rlength:
                break
            if k == 0:
                start = (s, s, None, None, 0, 0, None, None)
            out.append((e, e, None, None, 0, 0, None, None))
    else:
        for s, e in ctg2range:
            if s < rlength:
                continue
            if start is None:
                start = (None, None, s, s, 0, 0, None, None)
            out.append((None, None, e, e, 0, 0, None, None))
    if start is None:
        raise error("glocalchain: no sequence on axis %d" % axis)
    return start, out


def _glocal_pass_python(blocks, rlength, ctg2range, w, lastn, lastbp, axis):
    """one pass -> the indices into `blocks` of the chain, in chain order"""
    if axis not in (0, 1):
        raise error("glocalchain: axis is 0 or 1")
    if any(w[k] < 0 for k in _W):
        raise error("glocalchain: negative weight")
    n = len(blocks)
    if n == 0:
        return []
    c1, c2 = (0, 2) if axis == 0 else (2, 0)
    start, dummies = _glocal_dummies(rlength, ctg2range, axis)
    entries = [tuple(b) for b in blocks] + dummies
    m = len(entries)
    order = sorted(range(m), key=lambda i: (entries[i][c1], -entries[i][5]))       # stable: ties stay in input order, dummies behind
    H = [start] + [entries[i] for i in order]                                       # H[0] = start, H[k] = the k-th entry in sorted order
    score, back = [0] * (m + 1), [0] * (m + 1)
    deepest = 1
    for k in range(1, m + 1):
        b = H[k]
        while H[deepest][c1 + 1] < b[c1]:                                           # the first entry whose end reaches this block's begin
            deepest += 1
        far = H[deepest][c1]
        best, bp, l = None, 0, 0
        for p in range(k - 1, -1, -1):
            q = H[p]
            if q[6] is not None and b[6] is not None:
                if q[c1] == b[c1] or q[c1 + 1] >= b[c1 + 1]:
                    continue
                if q[c2] >= b[c2] and q[c2 + 1] <= b[c2 + 1]:
                    continue
            l += 1
            v = score[p] - _glocal_cost(q, b, ctg2range, w, axis)
            if best is None or v > best:                                            # ties: the predecessor met first, the nearest
                best, bp = v, p
            if b[c1] - q[c1] > lastbp and l >= lastn and q[c1] < far:
                break
        score[k] = best + w["alfa"] * b[5]
        back[k] = bp
    chain = []
    node = back[order.index(m - 1) + 1]                                             # `end` = the last dummy
    while node != 0:
        if H[node][6] is not None:
            chain.append(order[node - 1])
        node = back[node]
    return chain[::-1]


def glocalchain_python(blocks, rlength, qlength, ctg2range, rearrangecost=1000, inversioncost=1, lastn=50, lastbp=10000, axis=0, _lambda=5, eps=1, alfa=1,
                       gapopen=10):
    """the reference's glocalchain (useheap=False) restated: one pass over `blocks` on `axis` -> the chain, a new list; `blocks` is left as it is.
    Any non-negative weights, ints or floats, with Python's own arithmetic."""
    w = dict(rearrangecost=rearrangecost, inversioncost=inversioncost, _lambda=_lambda, eps=eps, alfa=alfa, gapopen=gapopen)
    return [blocks[i] for i in _glocal_pass_python(blocks, rlength, ctg2range, w, lastn, lastbp, axis)]


def _integral(kw):
    """the weights, lastn and lastbp as ints, or None where one of them is not integral"""
    out = {}
    for k in _W + ("lastn", "lastbp"):
        v = kw[k]
        if isinstance(v, float):
            if v != v or v in (float("inf"), float("-inf")) or v != int(v):
                return None
        out[k] = int(v)
    return out


_INFO_HEAD, _INFO_PASSES = 12, 64


_COLS = (("s1", np.int64), ("e1", np.int64), ("s2", np.int64), ("e2", np.int64), ("o", np.int32), ("score", np.int64), ("refid", np.int32), ("ctgid", np.int32))


def glocal_arrays(cols, rlength, ctg2range, axes=(0, 1), fixed=True, sa64=False, index=None, host=False, **kw):
    """the library's calls on columns: cols = dict of equally long arrays s1, e1, s2, e2, o, score, refid, ctgid (what getblocks_arrays gives, with o as
    an array); kw = integral weights, lastn, lastbp over GLOCAL_DEFAULTS.  fixed: every axis named to its fixed point (rv_glocal_filter), otherwise one pass
    per axis.  host: rv_glocal_host, no device is asked for; otherwise through `index` (or a fresh handle), whose switches choose the route.
    -> (the chain as indices into the columns, int32; info)"""
    kw = dict(GLOCAL_DEFAULTS, **kw)
    w = _integral(kw)
    if w is None:
        raise error("glocalchain: the library takes integral weights (glocalchain_python takes any)")
    mask = sum(1 << a for a in set(axes))
    if not mask or mask & ~3 or (not fixed and mask == 3):
        raise error("glocalchain: axes are 0 and 1; a single pass takes one of them")
    if not host and index is None:
        from . import reveallib, reveallib64
        index = (reveallib64 if sa64 else reveallib).index()
    lib = _lib.get(sa64) if host else index._lib
    arr = [np.ascontiguousarray(cols[k], dtype=dt) for k, dt in _COLS]
    n = len(arr[0])
    if any(len(a) != n for a in arr):
        raise error("glocalchain: columns of different lengths")
    rs = np.ascontiguousarray(np.array([int(s) for s, _ in ctg2range], dtype=np.int64))
    re = np.ascontiguousarray(np.array([int(e) for _, e in ctg2range], dtype=np.int64))
    par = np.array([w[k] for k in _W + ("lastn", "lastbp")], dtype=np.int64)
    info = np.zeros(_INFO_HEAD + _INFO_PASSES, dtype=np.int64)
    idx = np.zeros(max(n, 1), dtype=np.int32)
    head = (n, *[c.ctypes.data for c in arr], len(rs), rs.ctypes.data, re.ctypes.data, int(rlength), par.ctypes.data)
    if host:
        k = lib.dll.rv_glocal_host(*head, mask, 1 if fixed else 0, info.ctypes.data, len(info), idx.ctypes.data, max(n, 1))
    else:
        if fixed:
            k = lib.dll.rv_glocal_filter(index._h, *head, mask, info.ctypes.data, len(info))
        else:
            k = lib.dll.rv_glocal_blocks(index._h, *head, 0 if mask == 1 else 1, info.ctypes.data, len(info))
        if k >= 0 and lib.dll.rv_fetch_glocal(index._h, idx.ctypes.data, max(n, 1)) != 0:
            k = -1
    if k < 0:
        raise error(lib.err())
    return idx[:k], _glocal_info(info)


def _glocal_info(info):
    k = int(info[11])
    return dict(route="host" if info[0] else "device", passes=(int(info[1]), int(info[2])), after=[int(x) for x in info[_INFO_HEAD:_INFO_HEAD + min(k, _INFO_PASSES)]],
                tiles=int(info[3]), tiles_max=int(info[4]), chain_ms=info[5] / 1e6, chain_blocks=int(info[6]), bytes_up=int(info[7]), bytes_down=int(info[8]),
                edges=int(info[9]), sort_keys=int(info[10]))


def glocal_admit(blocks, rlength, qlength, ctg2range, **kw):
    """True where the library's 64-bit integer arithmetic takes these weights on this list (rv_glocal_admit): integral, and the largest possible
    |score| inside 62 bits.  A negative weight raises."""
    kw = dict(GLOCAL_DEFAULTS, **kw)
    if any(kw[k] < 0 for k in _W):
        raise error("glocalchain: negative weight")
    w = _integral(kw)
    if w is None or any(abs(v) >= 1 << 62 for v in w.values()):
        return False
    lib = _lib.get(False)
    maxc = max([int(e) for _, e in ctg2range] + [max(int(b[1]), int(b[3])) for b in blocks] + [0])
    maxs = max([int(b[5]) for b in blocks] + [0])
    if maxc >= 1 << 62 or maxs >= 1 << 62:
        return False
    par = np.array([w[k] for k in _W + ("lastn", "lastbp")], dtype=np.int64)
    r = lib.dll.rv_glocal_admit(len(blocks), len(ctg2range), maxc, maxs, par.ctypes.data)
    if r < 0:
        raise error(lib.err())
    return bool(r)


def _glocal_call(blocks, rlength, ctg2range, kw, axes, fixed, sa64, index, device):
    n = len(blocks)
    try:
        cols = {k: np.fromiter((int(b[c]) for b in blocks), dtype=dt, count=n) for c, (k, dt) in enumerate(_COLS)}
    except OverflowError:
        raise error("glocalchain: a block outside the library's integers")
    idx, info = glocal_arrays(cols, rlength, ctg2range, [a for a in (0, 1) if axes >> a & 1], fixed, sa64, index, not device, **kw)
    return [blocks[i] for i in idx.tolist()], info


def glocalchain_native(blocks, rlength, qlength, ctg2range, rearrangecost=1000, inversioncost=1, lastn=50, lastbp=10000, axis=0, _lambda=5, eps=1, alfa=1,
                       gapopen=10, sa64=False):
    """the same pass through the library's host C++ (rv_glocal_host): no device is asked for"""
    kw = dict(rearrangecost=rearrangecost, inversioncost=inversioncost, lastn=lastn, lastbp=lastbp, _lambda=_lambda, eps=eps, alfa=alfa, gapopen=gapopen)
    if axis not in (0, 1):
        raise error("glocalchain: axis is 0 or 1")
    return _glocal_call(blocks, rlength, ctg2range, kw, 1 << axis, False, sa64, None, False)[0]


def glocalchain_device(blocks, rlength, qlength, ctg2range, rearrangecost=1000, inversioncost=1, lastn=50, lastbp=10000, axis=0, _lambda=5, eps=1, alfa=1,
                       gapopen=10, sa64=False, index=None, info=False):
    """the same pass through the kernels (rv_glocal_blocks).  index: a handle that lends its stream, workspace and switches (constructed or not);
    without one a fresh index object is made for the call.  info=True: -> (chain, info)"""
    kw = dict(rearrangecost=rearrangecost, inversioncost=inversioncost, lastn=lastn, lastbp=lastbp, _lambda=_lambda, eps=eps, alfa=alfa, gapopen=gapopen)
    if axis not in (0, 1):
        raise error("glocalchain: axis is 0 or 1")
    r = _glocal_call(blocks, rlength, ctg2range, kw, 1 << axis, False, sa64, index, True)
    return r if info else r[0]


def glocal_filter(blocks, rlength, qlength, ctg2range, rearrangecost=10000, inversioncost=5, lastn=50, lastbp=20000, _lambda=3, eps=2, alfa=2, gapopen=1,
                  axes=(0, 1), sa64=False, index=None, route=None):
    """transform.py:307-356: glocalchain on the reference axis until a pass drops nothing, then the same on the query axis -> (chain, info).  The
    defaults are the command line's.  info: route ("device": the kernels, all passes in one call with a count per pass coming back; "host": the
    library's host C++, by RV_GLOCAL_HOST or for a list shorter than RV_GLOCAL_HOST_BELOW; "python": what rv_glocal_admit refuses), passes per axis,
    after = the blocks left by every pass.  route = "host" / "python" asks for that route (no device is asked for)."""
    kw = dict(rearrangecost=rearrangecost, inversioncost=inversioncost, lastn=lastn, lastbp=lastbp, _lambda=_lambda, eps=eps, alfa=alfa, gapopen=gapopen)
    mask = sum(1 << a for a in set(axes))
    if not mask or mask & ~3:
        raise error("glocal_filter: axes are 0 and 1")
    if route not in (None, "host", "python", "device"):
        raise error("glocal_filter: unknown route")
    admitted = glocal_admit(blocks, rlength, qlength, ctg2range, **kw)
    if route == "python" or not admitted:
        if route in ("host", "device"):
            raise error("glocal_filter: these weights are outside the library's integer arithmetic")
        cur, passes, after = list(blocks), [0, 0], []
        for a in (0, 1):
            if not mask >> a & 1:
                continue
            while True:
                nxt = glocalchain_python(cur, rlength, qlength, ctg2range, axis=a, **kw)
                passes[a] += 1
                after.append(len(nxt))
                dropped = len(nxt) != len(cur)
                cur = nxt
                if not dropped:
                    break
        return cur, dict(route="python", passes=tuple(passes), after=after)
    return _glocal_call(blocks, rlength, ctg2range, kw, mask, True, sa64, index, route != "host")


def synteny_chain(reference, contigs, minlength=20, cluster=True, maxdist=30, mincluster=50, minctglength=10000, rearrangecost=10000, inversioncost=5,
                  lastn=50, lastbp=20000, _lambda=3, eps=2, alfa=2, gapopen=1, sa64=False):
    """synteny_blocks + glocal_filter with the command line's defaults -> dict(chain = the list merge_consecutive is handed at transform.py:377,
    blocks = the list in front of the filter, ctg2range, sep, rlength, qlength, refnames, ctgnames, mums, info of glocal_filter)"""
    r = synteny_blocks(reference, contigs, minlength, cluster, maxdist, mincluster, minctglength, sa64)
    chain, info = glocal_filter(r["blocks"], r["rlength"], r["qlength"], r["ctg2range"], rearrangecost, inversioncost, lastn, lastbp, _lambda, eps, alfa,
                                gapopen, sa64=sa64)
    r.update(chain=chain, info=info)
    return r


# ---- merge_consecutive (transform.py:713-746); the rule: include/reveal_amd.h, rv_merge_blocks ---------------------------------------------------------
_MERGE_INFO = 9


def merge_consecutive_python(blocks):
    """the reference's merge_consecutive restated without its running head: neighbours of the reference order that are neighbours of the query order
    too, in the direction of their orientation and on one contig, fold into one block -> a new list in reference order; `blocks` is left as it is"""
    m = len(blocks)
    if m < 2:
        return list(blocks)
    R = sorted(blocks, key=lambda b: b[0])                                      # stable: ties keep the caller's order
    qinv = [0] * m
    for rank, i in enumerate(sorted(range(m), key=lambda i: R[i][2])):
        qinv[i] = rank
    out = []
    head, score = 0, R[0][5]
    for i in range(1, m + 1):
        if i < m:
            p, b = R[i - 1], R[i]
            if b[7] == p[7] and ((b[4] == p[4] == 0 and qinv[i] == qinv[i - 1] + 1) or (b[4] == p[4] == 1 and qinv[i] == qinv[i - 1] - 1)):
                score += b[5]
                continue
        h, t = R[head], R[i - 1]
        out.append((h[0], t[1], h[2], t[3], h[4], score, h[6], h[7]) if h[4] == 0 else (h[0], t[1], t[2], h[3], h[4], score, h[6], h[7]))
        if i < m:
            head, score = i, R[i][5]
    return out


def _columns(blocks, what):
    n = len(blocks)
    try:
        return {k: np.fromiter((int(b[c]) for b in blocks), dtype=dt, count=n) for c, (k, dt) in enumerate(_COLS)}
    except OverflowError:
        raise error("%s: a block outside the library's integers" % what)


def _rows(cols):
    return list(zip(*[np.asarray(cols[k]).tolist() for k, _ in _COLS]))


def _merge_info(info):
    return dict(route="host" if info[0] else "device", rows_in=int(info[1]), rows_out=int(info[2]), bytes_up=int(info[3]), bytes_down=int(info[4]),
                key_bits=(int(info[5]), int(info[6])), launches=int(info[7]), kernel_ms=info[8] / 1e6)


def merge_arrays(cols, sel=None, sa64=False, index=None, host=False):
    """the library's merge on columns: cols = dict of equally long arrays s1, e1, s2, e2, o, score, refid, ctgid; sel = the rows that make the list, in
    list order (int32 row numbers, duplicates allowed: the idx glocal_arrays returns), None = every row.  host: rv_merge_host, no device is asked for;
    otherwise rv_merge_blocks through `index` (or a fresh handle), whose switches choose the route.  -> (the merged list as a dict of columns, info)"""
    if not host and index is None:
        from . import reveallib, reveallib64
        index = (reveallib64 if sa64 else reveallib).index()
    lib = _lib.get(sa64) if host else index._lib
    arr = [np.ascontiguousarray(cols[k], dtype=dt) for k, dt in _COLS]
    n = len(arr[0])
    if any(a.ndim != 1 or len(a) != n for a in arr):
        raise error("merge: columns of different lengths")
    if sel is None:
        m, psel = n, None
    else:
        s = np.asarray(sel)
        if s.ndim != 1 or (len(s) and s.dtype.kind not in "iu"):
            raise error("merge: sel is a list of row numbers")
        if len(s) and (int(s.min()) < 0 or int(s.max()) >= n):
            raise error("merge: sel names a row outside 0 .. %d" % n)
        m = len(s)
        s = np.ascontiguousarray(s, dtype=np.int32) if m else np.zeros(1, dtype=np.int32)       # (an empty sel is still a sel: a pointer, not NULL)
        psel = s.ctypes.data
    info = np.zeros(_MERGE_INFO, dtype=np.int64)
    out = [np.zeros(max(m, 1), dtype=dt) for _, dt in _COLS]
    head = (n, *[c.ctypes.data for c in arr], m, psel, info.ctypes.data, len(info))
    if host:
        k = lib.dll.rv_merge_host(*head, *[c.ctypes.data for c in out], max(m, 1))
    else:
        k = lib.dll.rv_merge_blocks(index._h, *head)
        if k >= 0 and lib.dll.rv_fetch_merge(index._h, *[c.ctypes.data for c in out], max(m, 1)) != 0:
            k = -1
    if k < 0:
        raise error(lib.err())
    return {name: c[:k] for (name, _), c in zip(_COLS, out)}, _merge_info(info)


def merge_consecutive_native(blocks, sa64=False):
    """the same through the library's host C++ (rv_merge_host): no device is asked for"""
    return _rows(merge_arrays(_columns(blocks, "merge"), None, sa64, None, True)[0])


def merge_consecutive_device(blocks, sa64=False, index=None, info=False):
    """the same through rv_merge_blocks: the kernels, or the host rule where the handle's switches say so (RV_MERGE_HOST, RV_MERGE_HOST_BELOW).
    index: a handle that lends its stream, workspace and switches; without one a fresh index object is made.  info=True: -> (list, info)"""
    cols, i = merge_arrays(_columns(blocks, "merge"), None, sa64, index, False)
    return (_rows(cols), i) if info else _rows(cols)


# ---- the chain's tail (transform.py:376-435, 528-530): overlap removal, chainscore, optimise, extendblocks -------------------------------------------
def _trim(b, overlap, coord, front):
    """block b with `overlap` taken off its front (front=True) or its end on the axis of `coord`, the other axis following the orientation"""
    s1, e1, s2, e2, o, score, refid, ctgid = b
    left = score - overlap if overlap < score else 0
    if front:
        if o == 0:
            return (s1 + overlap, e1, s2 + overlap, e2, o, left, refid, ctgid)
        return (s1 + overlap, e1, s2, e2 - overlap, o, left, refid, ctgid) if coord == 0 else (s1, e1 - overlap, s2 + overlap, e2, o, left, refid, ctgid)
    if o == 0:
        return (s1, e1 - overlap, s2, e2 - overlap, o, left, refid, ctgid)
    return (s1, e1 - overlap, s2 + overlap, e2, o, left, refid, ctgid) if coord == 0 else (s1 + overlap, e1, s2, e2 - overlap, o, left, refid, ctgid)


def remove_overlap_python(blocks, greedy=False):
    """remove_overlap_conservative_blocks (transform.py:1334-1400) or, greedy=True, remove_overlap_greedy_blocks (:1402-1485): on the reference axis and
    then on the query axis, contained blocks leave and an overlap of two neighbours is taken off one of them -> a new list.  Where the reference
    raises (its pop loop empties the list: IndexError; one of its asserts), this raises transform.error."""
    anchors = [tuple(b) for b in blocks]
    for coord in (0, 2):
        if len(anchors) <= 1:
            return anchors
        anchors.sort(key=lambda m: (m[coord], (m[coord + 1] - m[coord]) * -1))
        kept = [anchors[0]]
        last = anchors[0]
        for a in anchors[1:]:
            if a[coord] < last[coord + 1] and a[coord + 1] <= last[coord + 1]:        # contained
                continue
            kept.append(a)
            last = a
        anchors = kept
        out = [anchors[0]]
        for a in anchors[1:]:
            score = a[5]
            prev = out[-1]
            pl, pscore = prev[1] - prev[0], prev[5]
            overlap = prev[coord + 1] - a[coord]
            if overlap > 0:
                if not greedy or pscore > score:                                     # the block itself gives the overlap up
                    if score <= overlap:
                        continue
                    a = _trim(a, overlap, coord, True)
                    if greedy:
                        out.append(a)
                        continue
                    if not a[coord + 1] > prev[coord + 1]:
                        raise error("remove_overlap: a trimmed block ends inside the one in front of it")
                while pl <= overlap or pscore <= overlap:
                    out.pop()
                    if not out:
                        raise error("remove_overlap: no block left in front of an overlap")
                    prev = out[-1]
                    pscore = prev[5]
                    overlap = prev[coord + 1] - a[coord]
                    if overlap < 0:
                        break
                    pl = prev[1] - prev[0]
                if overlap > 0:
                    if greedy and not (pl > overlap and pscore > overlap):
                        raise error("remove_overlap: an overlap as long as the block in front of it")
                    if pscore - overlap < 0:
                        raise error("remove_overlap: an overlap above the score of the block in front of it")
                    out[-1] = _trim(prev, overlap, coord, False)
            out.append(a)
        anchors = out
    return anchors


def _orders(chain):
    """the chain stably sorted by s1, its query order (positions into the sorted chain) and the inverse of that"""
    C = sorted(chain, key=lambda s: s[0])
    qryorder = sorted(range(len(C)), key=lambda i: C[i][2])
    inv = [0] * len(C)
    for rank, i in enumerate(qryorder):
        inv[i] = rank
    return C, qryorder, inv


def chainscore_python(chain, rlength, qlength, ctg2range, rearrangecost=1000, inversioncost=1, _lambda=5, eps=1, alfa=1, gapopen=10):
    """the reference's chainscore (transform.py:836-935) -> (weight, cost, edgecosts); `chain` is left as it is (the reference sorts it in place).  A
    plain step from one contig to the next costs gapopen in edgecosts and nothing in cost, as in the reference."""
    w = dict(rearrangecost=rearrangecost, inversioncost=inversioncost, _lambda=_lambda, eps=eps, gapopen=gapopen)
    if len(chain) == 0:
        cost = _gapcost((0, 0, rlength, rlength, 0), (rlength, rlength, rlength + qlength, rlength + qlength, 0), w, 0, 2)
        return 0, cost, [cost]
    C, qryorder, inv = _orders(chain)
    o0 = C[0][4]
    fs, fe = ctg2range[C[0][7]]
    ls, le = ctg2range[C[-1][7]]
    start = (0, 0, fs, fs, o0) if o0 == 0 else (0, 0, fe, fe, o0)
    end = (rlength, rlength, le, le, o0) if o0 == 0 else (rlength, rlength, ls, ls, o0)
    if C[-1][0] > rlength:
        raise error("chainscore: a block begins behind rlength")
    cost = _gapcost(start, C[0], w, 0, 2)
    edgecosts = [cost]
    weight = alfa * C[0][5]
    n = len(C)
    for ri in range(1, n):
        p, b = C[ri - 1], C[ri]
        weight += alfa * b[5]
        pqi, qi = inv[ri - 1], inv[ri]
        if p[7] == b[7] and p[6] == b[6]:
            gc = _gapcost(p, b, w, 0, 2) if (pqi == qi - 1 or pqi == qi + 1) else gapopen + rearrangecost
            cost += gc
            edgecosts.append(gc)
            continue
        if b[4] == 0:
            pq_ctg = C[qryorder[qi - 1]][7] if qi > 0 else "start"
        else:
            pq_ctg = C[qryorder[qi + 1]][7] if qi < n - 1 else "end"
        if p[4] == 0:
            nq_ctg = C[qryorder[pqi + 1]][7] if pqi < n - 1 else "end"
        else:
            nq_ctg = C[qryorder[pqi - 1]][7] if pqi > 0 else "start"
        if pq_ctg == b[7] or nq_ctg == p[7]:
            cost += gapopen + rearrangecost
            edgecosts.append(gapopen + rearrangecost)
        else:
            edgecosts.append(gapopen)
    endcost = _gapcost(C[-1], end, w, 0, 2)
    cost += endcost
    edgecosts.append(endcost)
    return weight, cost, edgecosts


def optimise_python(blocks, rlength, qlength, ctg2range, rearrangecost=1000, inversioncost=1, _lambda=5, eps=1, alfa=1, gapopen=10):
    """one sweep of the reference's optimise (transform.py:801-834): the candidates in ascending score (ties in incoming order); a candidate whose
    chain scores not lower without it is dropped for good -> (chain in reference order, weight, cost, edgecosts); `blocks` is left as it is"""
    kw = dict(rearrangecost=rearrangecost, inversioncost=inversioncost, _lambda=_lambda, eps=eps, alfa=alfa, gapopen=gapopen)
    org = sorted(blocks, key=lambda c: c[5])
    best = sorted(blocks, key=lambda s: s[0])
    bw, bc, be = chainscore_python(best, rlength, qlength, ctg2range, **kw)
    stack = []
    for i in range(len(org)):
        tmp = stack + org[i + 1:]
        w, c, e = chainscore_python(tmp, rlength, qlength, ctg2range, **kw)
        if w - c < bw - bc:
            stack.append(org[i])
        else:
            best, bw, bc, be = sorted(tmp, key=lambda s: s[0]), w, c, e
    return best, bw, bc, be


def _tail_admit(blocks, rlength, qlength, ctg2range, kw):
    """the weights as ints where the library's 64-bit arithmetic takes them on this list, else None"""
    w = _integral(dict(kw, lastn=0, lastbp=0))
    if w is None or any(v < 0 or v >= 1 << 62 for v in w.values()):
        return None
    try:
        vals = [int(rlength) + int(qlength)] + [int(x) for r in ctg2range for x in r] + [int(x) for b in blocks for x in b[:4]]
        maxs = sum(int(b[5]) for b in blocks)                                      # (what merge_consecutive can make of them)
    except (TypeError, ValueError):
        return None
    if min(vals) < 0 or max(vals) >= 1 << 61 or maxs >= 1 << 61 or any(int(b[5]) < 0 for b in blocks):
        return None
    par = np.array([w[k] for k in _W + ("lastn", "lastbp")], dtype=np.int64)
    if _lib.get(False).dll.rv_glocal_admit(len(blocks), len(ctg2range), max(vals), maxs, par.ctypes.data) != 1:
        return None
    return w


def _tail_call(fn, blocks, rlength, qlength, ctg2range, w, sa64):
    lib = _lib.get(sa64)
    cols = _columns(blocks, "chainscore")
    arr = [cols[k] for k, _ in _COLS]
    rs = np.ascontiguousarray(np.array([int(s) for s, _ in ctg2range], dtype=np.int64))
    re = np.ascontiguousarray(np.array([int(e) for _, e in ctg2range], dtype=np.int64))
    par = np.array([w[k] for k in _W] + [0, 0], dtype=np.int64)
    wc = np.zeros(2, dtype=np.int64)
    n = len(blocks)
    res = np.zeros(n + 1, dtype=np.int64 if fn == "rv_chainscore_host" else np.int32)
    k = getattr(lib.dll, fn)(n, *[c.ctypes.data for c in arr], len(rs), rs.ctypes.data, re.ctypes.data, int(rlength), int(qlength), par.ctypes.data, wc.ctypes.data,
                             res.ctypes.data, n + 1)
    if k < 0:
        raise error(lib.err())
    return int(wc[0]), int(wc[1]), res[:k].tolist()


def chainscore_native(chain, rlength, qlength, ctg2range, rearrangecost=1000, inversioncost=1, _lambda=5, eps=1, alfa=1, gapopen=10, sa64=False):
    """chainscore through the library's host C++ (rv_chainscore_host); integral weights inside rv_glocal_admit's bound, anything else raises"""
    kw = dict(rearrangecost=rearrangecost, inversioncost=inversioncost, _lambda=_lambda, eps=eps, alfa=alfa, gapopen=gapopen)
    w = _tail_admit(chain, rlength, qlength, ctg2range, kw)
    if w is None:
        raise error("chainscore: these weights are outside the library's integer arithmetic")
    return _tail_call("rv_chainscore_host", chain, rlength, qlength, ctg2range, w, sa64)


def optimise_native(blocks, rlength, qlength, ctg2range, rearrangecost=1000, inversioncost=1, _lambda=5, eps=1, alfa=1, gapopen=10, sa64=False):
    """one sweep through the library's host C++ (rv_optimise_host: both orders made once, a candidate skipped in them) -> as optimise_python"""
    kw = dict(rearrangecost=rearrangecost, inversioncost=inversioncost, _lambda=_lambda, eps=eps, alfa=alfa, gapopen=gapopen)
    w = _tail_admit(blocks, rlength, qlength, ctg2range, kw)
    if w is None:
        raise error("optimise: these weights are outside the library's integer arithmetic")
    bw, bc, idx = _tail_call("rv_optimise_host", blocks, rlength, qlength, ctg2range, w, sa64)
    best = [tuple(blocks[i]) for i in idx]
    return best, bw, bc, _tail_call("rv_chainscore_host", best, rlength, qlength, ctg2range, w, sa64)[2]


def optimise_loop(blocks, rlength, qlength, ctg2range, rearrangecost=1000, inversioncost=1, _lambda=5, eps=1, alfa=1, gapopen=10, route="python", sa64=False):
    """the loop of transform.py:404-433: sweeps until one does not raise the score, merge_consecutive behind every accepted one
    -> (blocks, weight, cost, edgecosts, accepted sweeps).  route: "python" or "host" (the library's host C++)."""
    kw = dict(rearrangecost=rearrangecost, inversioncost=inversioncost, _lambda=_lambda, eps=eps, alfa=alfa, gapopen=gapopen)
    score_fn, sweep_fn, merge_fn = (chainscore_python, optimise_python, merge_consecutive_python) if route == "python" else (
        lambda *a, **k: chainscore_native(*a, sa64=sa64, **k), lambda *a, **k: optimise_native(*a, sa64=sa64, **k), lambda b: merge_consecutive_native(b, sa64))
    blocks = sorted(blocks, key=lambda s: s[0])
    weight, cost, edgecosts = score_fn(blocks, rlength, qlength, ctg2range, **kw)
    score, sweeps = weight - cost, 0
    while True:
        t, tw, tc, te = sweep_fn(blocks, rlength, qlength, ctg2range, **kw)
        if tw - tc <= score:
            break
        score, weight, cost, edgecosts = tw - tc, tw, tc, te
        blocks = merge_fn(t)
        sweeps += 1
    return blocks, weight, cost, edgecosts, sweeps


def extendblocks_python(blocks, ctg2range):
    """the reference's extendblocks (transform.py:748-799): every block grows to the end of its neighbour in front and half-way (floor) to the one
    behind it, or to the ends of its sequence, on the reference axis and then on the query axis -> a new list in query order, as the reference
    leaves it.  A block that ends up empty raises transform.error (the reference's assert)."""
    B = sorted((tuple(b) for b in blocks), key=lambda s: s[0])
    for axis, (c, ident) in enumerate(((0, 6), (2, 7))):
        if axis == 1:
            B.sort(key=lambda s: s[2])
        n = len(B)
        for i in range(n):
            blk = list(B[i])
            seq = blk[ident]
            s, e = blk[c], blk[c + 1]
            s = B[i - 1][c + 1] if i > 0 and B[i - 1][ident] == seq else ctg2range[seq][0]          # (B[i-1] has been extended already)
            if i < n - 1 and B[i + 1][ident] == seq:
                e += (B[i + 1][c] - e) // 2
            else:
                e = ctg2range[seq][1]
            if not s < e:
                raise error("extendblocks: an empty block on the %s axis" % ("reference" if axis == 0 else "query"))
            blk[c], blk[c + 1] = s, e
            B[i] = tuple(blk)
    return B


def chain_tail(chain, rlength, qlength, ctg2range, greedy=False, minchainsum=50, optimise=True, rearrangecost=10000, inversioncost=5, _lambda=3, eps=2, alfa=2,
               gapopen=1, route=None, sa64=False, merged=False):
    """transform.py:376-435 and 528-530 on the chain glocal_filter leaves: merge_consecutive, overlap removal (conservative, or greedy), blocks below
    minchainsum dropped, merge_consecutive, the optimise loop where more than one block is left, merge_consecutive, chainscore, extendblocks.  The
    weights default to the command line's.  route: None = the library's host C++ where rv_glocal_admit takes the weights on this list and Python's
    arithmetic where not, "host" / "python" ask for one of them.  merged=True: `chain` has been through the first merge_consecutive already.
    -> dict(blocks = the chain in reference order before extension (what the bed file reads), weight, cost, edgecosts, extended = the list of
    extendblocks, info = dict(route, sweeps, stages = the list behind every stage))"""
    kw = dict(rearrangecost=rearrangecost, inversioncost=inversioncost, _lambda=_lambda, eps=eps, alfa=alfa, gapopen=gapopen)
    if route not in (None, "host", "python"):
        raise error("chain_tail: unknown route")
    if any(kw[k] < 0 for k in _W):
        raise error("chain_tail: negative weight")
    chain = [tuple(b) for b in chain]
    stages = {}

    def admitted(blocks):
        return route != "python" and _tail_admit(blocks, rlength, qlength, ctg2range, kw) is not None

    native = admitted(chain)
    if route == "host" and not native:
        raise error("chain_tail: these weights are outside the library's integer arithmetic")
    merge = (lambda b: merge_consecutive_native(b, sa64)) if native else merge_consecutive_python
    cur = chain if merged else merge(chain)
    stages["merged"] = list(cur)
    cur = remove_overlap_python(cur, greedy)
    stages["overlap"] = list(cur)
    cur = [b for b in cur if b[5] >= minchainsum]
    stages["filtered"] = list(cur)
    cur = merge(cur)
    stages["merged2"] = list(cur)
    sweeps = 0
    if optimise and len(cur) > 1:
        cur, _, _, _, sweeps = optimise_loop(cur, rlength, qlength, ctg2range, route="host" if native else "python", sa64=sa64, **kw)
        stages["optimised"] = list(cur)
    cur = merge(cur)
    weight, cost, edgecosts = (chainscore_native(cur, rlength, qlength, ctg2range, sa64=sa64, **kw) if native else
                               chainscore_python(cur, rlength, qlength, ctg2range, **kw))
    cur = sorted(cur, key=lambda s: s[0])
    return dict(blocks=cur, weight=weight, cost=cost, edgecosts=edgecosts, extended=extendblocks_python(cur, ctg2range),
                info=dict(route="host" if native else "python", sweeps=sweeps, stages=stages))


def synteny_layout(reference, contigs, minlength=20, cluster=True, maxdist=30, mincluster=50, minctglength=10000, rearrangecost=10000, inversioncost=5,
                   lastn=50, lastbp=20000, _lambda=3, eps=2, alfa=2, gapopen=1, greedy=False, minchainsum=50, optimise=True, sa64=False):
    """reference and contigs -> the layout `reveal transform` writes its bed file and builds its breakpoint graph from: synteny_chain's stages and
    chain_tail in one call, the block list staying in columns from getblocks through the glocal filter until merge_consecutive (rv_merge_blocks, the
    filter's chain as `sel`) has made it small; only the merged rows become tuples.  -> chain_tail's dict plus ctg2range, sep, rlength, qlength,
    refnames, ctgnames, mums, and info with `glocal` and `merge` (the two calls' own info) and `blocks` (the rows in front of the filter)"""
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
        raise error("synteny_layout: no sequence of at least minctglength in %s" % ("the reference" if not names[0] else "the contigs"))
    idx.construct(rc=0)
    fwd = idx.getblocks_arrays(minlength, cluster, maxdist, mincluster)
    idx.construct(rc=1)
    rc = idx.getblocks_arrays(minlength, cluster, maxdist, mincluster)
    sep, n = idx.nsep[0], idx.n
    cols = {k: np.concatenate([np.asarray(fwd[k], dtype=dt), np.asarray(rc[k], dtype=dt)]) for k, dt in _COLS if k != "o"}
    cols["o"] = np.concatenate([np.zeros(len(fwd["s1"]), dtype=np.int32), np.ones(len(rc["s1"]), dtype=np.int32)])
    rlength, qlength = sep, n - sep
    kw = dict(rearrangecost=rearrangecost, inversioncost=inversioncost, lastn=lastn, lastbp=lastbp, _lambda=_lambda, eps=eps, alfa=alfa, gapopen=gapopen)
    if _integral(kw) is None:
        raise error("synteny_layout: the column pipeline takes integral weights (synteny_chain + chain_tail take any)")
    sel, ginfo = glocal_arrays(cols, rlength, ctg2range, (0, 1), True, sa64, idx, False, **kw)
    mcols, minfo = merge_arrays(cols, sel, sa64, idx, False)
    tail = {k: kw[k] for k in _W}
    r = chain_tail(_rows(mcols), rlength, qlength, ctg2range, greedy, minchainsum, optimise, sa64=sa64, merged=True, **tail)
    r["info"].update(glocal=ginfo, merge=minfo, blocks=len(cols["s1"]))
    r.update(ctg2range=ctg2range, sep=sep, rlength=rlength, qlength=qlength, refnames=names[0], ctgnames=names[1], mums=(fwd["info"]["mums"], rc["info"]["mums"]))
    return r
