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

Not done here: merge_consecutive, remove_overlap_*, optimise / chainscore, extendblocks, the bed file and the breakpoint graph (host work on the few
blocks that survive); useheap; non-integral weights outside Python; the getblocks output kept in device memory across construct(rc=1); --cutn, a
reverse complement made on the device, a form for many inputs at once.
"""
from bisect import bisect_left

import numpy as np

from . import _lib
from .reveallib import error

__all__ = ["blocks_python", "blocks_native", "blocks_device", "synteny_blocks", "glocalchain_python", "glocalchain_native", "glocalchain_device",
           "glocal_filter", "glocal_arrays", "glocal_admit", "synteny_chain", "error"]


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
