"""The collinear chain of `reveal chain` for many jobs at once (include/reveal_amd.h rv_many_kchain, csrc/rv_kchain.hip).

`reveal chain --recurse` (reveal/chain.py:57-124) builds a fresh index per gap and hands its getmums / getmultimums(minn=k) list to `chain()`
(chain.py:214-314): the matches in all k sequences, capped at maxmums, a k-dimensional collinear-chaining programme with `gapcost`, the best path; its
gaps are the next level's jobs.  `kchain_many` does that for every job of a call: the scan of `mums_many`, then each list chained on the device where
the write pass has left it; only the paths come back.  A job the kernel does not take (more than 2048 members or RV_KCHAIN_CAP records, a job the scan
runs the ordinary way) is prepared on the host inside the call (the cap, the points, the order of the targets, the kd order); with at least
RV_KCHAIN_BIG_MIN kept points its programme then runs in device memory, tile by tile, together with every other such list of the call
(csrc/rv_kchain_big.hip: up to 2^20 points), otherwise -- or where the preparation refuses the list, see include/reveal_amd.h -- on the host
(`rv_kchain`).  The results do not depend on the path.  `kchain_device` chains lists the caller brings the same way, with no scan.  Ties between
predecessors of equal score are decided as the reference decides them: by the order in which `range_search` hands out the leaves of `kdtree` (`kd_order`).

The one deliberate departure: a job of TWO sequences.  The reference's `getmums` returns `(l, (a, b), rc)`, `chain()`'s filter `m[1] == k` drops every
such record, and a two-genome `reveal chain` anchors nothing.  The function plainly intends the multi-MUM shape `(l, 2, ((0, a), (1, b)))`
(reveal.c:167; `mums_many(kind="multimums")` gives it): pairs are chained from that shape.

Positions of a path are relative to each sequence's begin (the reference's coordinates with `offsets` all zero).  Scores are 64-bit, weights 0 .. 2^20.
`kchain_python`, `rv_kchain` and the programme in device memory are O(m^2 k^2) per job with no tree; the last spreads it over the device.
"""
import ctypes

import numpy as np

from . import _lib, many
from .many import Batch, error

GCMODELS = {"sumofpairs": 0, "star-avg": 1, "star-med": 2}
KCHAIN_MEMBERS = 2048      # RV_KCHAIN_MEMBERS: members (records x k) of the largest job the kernel chains
KCHAIN_CAP = 1024          # RV_KCHAIN_CAP: ... and its records (the switch of that name lowers it)
KCHAIN_WMAX = 1 << 20      # RV_KCHAIN_WMAX
KCHAIN_FLAG = 4            # bit of `Batch.flagged()` of a job the kernel gave back to the host
KCHAIN_BIG_TILE = 64       # RV_KCHAIN_BIG_TILE: targets of a tile of the programme in device memory
KCHAIN_BIG_CAP = 1 << 20   # RV_KCHAIN_BIG_CAP: kept points of the longest list it takes
KCHAIN_BIG_MIN = 512        # default of the switch RV_KCHAIN_BIG_MIN: kept points from which a list the kernel above did not chain goes there (1 .. 1025)
# rv_kchain_admit: why the preparation leaves a list to the host programme
KCHAIN_REFUSE = {"l0": 1, "shared": 2, "bits": 4, "cap": 8, "k": 16, "score": 32}


# ---- plain Python restatement ----
def gapcost(a, b, model="sumofpairs"):
    """utils.gapcost (utils.py:162-183) with Python 2's integer division"""
    k = len(a)
    if model == "star-avg":
        return abs(sum(a[i] - b[i] for i in range(k))) // k
    D = [abs(a[i] - b[i]) for i in range(k)]
    if model == "star-med":
        return sorted(D)[k // 2]
    if model != "sumofpairs":
        raise error("unknown gap cost model %r (%s)" % (model, ", ".join(sorted(GCMODELS))))
    return sum(abs(D[i] - D[j]) for i in range(k) for j in range(i + 1, k))


def kd_order(points, k):
    """the order in which utils.range_search hands out the leaves of utils.kdtree(points, k): right subtree first.  points: in list order"""
    out = []
    stack = [(list(points), 0)]
    while stack:
        pts, depth = stack.pop()
        n = len(pts)
        if n == 0:
            continue
        if n == 1:
            out.append(pts[0])
            continue
        if depth > 8192:
            raise error("identical points (the reference's kdtree does not end on them)")
        d = depth % k
        sp = sorted(pts, key=lambda p: p[d])
        split = sp[n // 2][d]
        if split == sp[0][d]:
            split += 1
        stack.append(([p for p in sp if p[d] < split], depth + 1))      # (popped last: the left subtree follows the right one)
        stack.append(([p for p in sp if p[d] >= split], depth + 1))
    return out


def kchain_python(records, lens, maxmums=0, wpen=1, wscore=1, gcmodel="sumofpairs", tie="kd"):
    """chain() for one job.  records: [(l, n, ((sample, pos), ..)), ..] in emission order, positions in the coordinates of the job's text `s0$s1$..`;
    lens: the k sequence lengths.  -> (path, end_score): path = [(l, (p0 .. pk-1), score), ..] without the two sentinels.  tie: "kd" -- the
    reference's rule; "dim0" -- candidates of equal score in the order of their first coordinate instead (for tests that show the rule decides)."""
    k = len(lens)
    begin = [sum(lens[:d]) + d for d in range(k)]
    mums = [r for r in records if r[1] == k]
    if len(mums) > maxmums and maxmums != 0:
        mums = sorted(mums, key=lambda r: r[0])[-maxmums:]
    else:
        mums = sorted(mums, key=lambda r: r[0])
    p1, p2 = tuple([-1] * k), tuple(int(x) for x in lens)
    if not mums:
        return [], -wpen * gapcost(p1, p2, gcmodel)
    length, points = {}, []
    for l, _, mem in mums:
        pt = sorted(p for _, p in mem)
        pt = tuple(pt[d] - begin[d] for d in range(k))
        points.append(pt)
        length[pt] = l
    length[p2] = 0
    points.append(p2)
    points = sorted(points, key=lambda p: p[0])
    order = kd_order(points, k) if tie == "kd" else list(points)
    score, back = {p2: 0}, {}
    gain = k * (k - 1) // 2
    for t in points:
        best, bs = p1, -wpen * gapcost(p1, t, gcmodel)
        for v in order:
            if v == t:
                continue
            lv = length[v]
            if any(v[d] > t[d] or v[d] + lv > t[d] for d in range(k)):
                continue
            sc = score[v] + wscore * (lv * gain) - wpen * gapcost(v, t, gcmodel)
            if sc > bs:
                bs, best = sc, v
        score[t], back[t] = bs, best
    path, v = [], back[p2]
    while v != p1:
        path.append((length[v], v, score[v]))
        v = back[v]
    return path[::-1], score[p2]


def kchain_native(records, lens, maxmums=0, wpen=1, wscore=1, gcmodel="sumofpairs", sa64=False):
    """the same through `rv_kchain` (host C++; no device is asked for)"""
    lib = _lib.get(sa64)
    k = len(lens)
    nrec = len(records)
    l = np.array([r[0] for r in records] or [0], np.uint32)
    n = np.array([r[1] for r in records] or [0], np.int32)
    off = np.zeros(nrec + 1, np.int64)
    for i, r in enumerate(records):
        off[i + 1] = off[i] + len(r[2])
    so = np.array([s for r in records for s, _ in r[2]] or [0], np.uint16)
    pos = np.array([p for r in records for _, p in r[2]] or [0], np.int64)
    ln = np.array(lens, np.int64)
    ol = np.zeros(max(nrec, 1), np.uint32); op = np.zeros(max(nrec, 1) * k, np.int64); osc = np.zeros(max(nrec, 1), np.int64)
    end = ctypes.c_int64(0)
    nn = lib.dll.rv_kchain(k, nrec, l.ctypes.data, n.ctypes.data, off.ctypes.data, so.ctypes.data, pos.ctypes.data, ln.ctypes.data, int(maxmums), int(wpen),
                           int(wscore), GCMODELS[gcmodel], ol.ctypes.data, op.ctypes.data, osc.ctypes.data, ctypes.addressof(end))
    if nn < 0:
        raise error(lib.err())
    return [(int(ol[x]), tuple(int(p) for p in op[x * k:(x + 1) * k]), int(osc[x])) for x in range(nn)], int(end.value)


def _pack_lists(lists):
    """[(records, lens), ..] -> the arrays of rv_many_kchain_lists (records of all lists back to back)"""
    ks = np.array([len(lens) for _, lens in lists] or [0], np.int32)
    nrec = np.array([len(recs) for recs, _ in lists] or [0], np.int64)
    allrec = [r for recs, _ in lists for r in recs]
    l = np.array([r[0] for r in allrec] or [0], np.uint32)
    n = np.array([r[1] for r in allrec] or [0], np.int32)
    off = np.zeros(len(allrec) + 1, np.int64)
    np.cumsum([len(r[2]) for r in allrec], out=off[1:])
    so = np.array([s for r in allrec for s, _ in r[2]] or [0], np.uint16)
    pos = np.array([p for r in allrec for _, p in r[2]] or [0], np.int64)
    ln = np.array([x for _, lens in lists for x in lens] or [0], np.int64)
    return ks, nrec, l, n, off, so, pos, ln


def kchain_admit(records, lens, maxmums=0, wpen=1, wscore=1, sa64=False):
    """rv_kchain_admit (host C++; no device is asked for): the KCHAIN_REFUSE bits for which the preparation leaves this list to the host programme; 0: the
    device programme takes it"""
    lib = _lib.get(sa64)
    ks, nrec, l, n, off, so, pos, ln = _pack_lists([(records, lens)])
    r = lib.dll.rv_kchain_admit(len(lens), len(records), l.ctypes.data, n.ctypes.data, off.ctypes.data, pos.ctypes.data, ln.ctypes.data, int(maxmums), int(wpen), int(wscore))
    if r < 0:
        raise error(lib.err())
    return r


def kchain_device(lists, maxmums=0, wpen=1, wscore=1, gcmodel="sumofpairs", sa64=False, batch=None, big_min=None):
    """rv_many_kchain_lists: chain() for lists the caller brings, with no scan.  lists: [(records, lens), ..] as for `kchain_python`.  -> ([(path,
    end_score), ..], info): info = dict(lists, big, host, big_launches): `big` lists ran the programme in device memory (all of them in the same
    `big_launches` launches: the tiles of the longest), `host` on the host.  `big_min`: sets the switch RV_KCHAIN_BIG_MIN of the batch (kept points from
    which a list goes to the device; default KCHAIN_BIG_MIN)."""
    if gcmodel not in GCMODELS:
        raise error("unknown gap cost model %r (%s)" % (gcmodel, ", ".join(sorted(GCMODELS))))
    if int(maxmums) < 0:
        raise error("maxmums >= 0")
    if not (0 <= int(wpen) <= KCHAIN_WMAX and 0 <= int(wscore) <= KCHAIN_WMAX):
        raise error("weights of 0 .. 2^20")
    lists = [(list(recs), [int(x) for x in lens]) for recs, lens in lists]
    if any(len(lens) < 2 for _, lens in lists):
        raise error("a list needs at least two sequences")
    b = batch if batch is not None else Batch(sa64)
    if big_min is not None:
        b.option("RV_KCHAIN_BIG_MIN", int(big_min))
    ks, nrec, l, n, off, so, pos, ln = _pack_lists(lists)
    if b._dll.rv_many_kchain_lists(b._m, len(lists), ks.ctypes.data, nrec.ctypes.data, l.ctypes.data, n.ctypes.data, off.ctypes.data, so.ctypes.data, pos.ctypes.data,
                                   ln.ctypes.data, int(maxmums), int(wpen), int(wscore), GCMODELS[gcmodel]) != 0:
        b._fail()
    chains = Chains(b.chains(len(lists)), [len(lens) for _, lens in lists])
    big = b.kchain_big()
    info = dict(lists=len(lists), big=big[0], host=len(lists) - big[0], big_launches=big[1])
    return [(chains[j], int(chains.end_score[j])) for j in range(len(lists))], info


# ---- the batch ----
def _batch_kchain_big(self):
    """rv_many_kchain_big -> (lists of the last kchain call the programme in device memory chained, its step launches)"""
    o = (ctypes.c_int64 * 2)()
    if self._dll.rv_many_kchain_big(self._m, o) != 0:
        self._fail()
    return int(o[0]), int(o[1])


def _batch_kchain(self, minlength=20, maxmums=0, wpen=1, wscore=1, gcmodel="sumofpairs"):
    """rv_many_kchain: the chain of every job instead of its match list.  The jobs stay; the result of an earlier run() or scan() does not."""
    if gcmodel not in GCMODELS:
        raise error("unknown gap cost model %r (%s)" % (gcmodel, ", ".join(sorted(GCMODELS))))
    if self._dll.rv_many_kchain(self._m, int(minlength), int(maxmums), int(wpen), int(wscore), GCMODELS[gcmodel]) != 0:
        self._fail()


def _batch_chains(self, nlists=None):
    """-> (first[jobs + 1], l, score, pos, end_score): job j owns the nodes first[j] .. first[j+1] of l / score; the positions of ALL nodes lie back
    to back in pos, k of job j for each of its nodes, in sequence order and relative to each sequence's begin.  nlists: after rv_many_kchain_lists,
    whose lists are not the batch's jobs"""
    nj = len(self._lens) if nlists is None else int(nlists)
    first = np.zeros(nj + 1, np.int64)
    mem = ctypes.c_int64(0)
    nn = self._dll.rv_many_kchain_count(self._m, first.ctypes.data, ctypes.byref(mem))
    if nn < 0:
        self._fail()
    l = np.zeros(max(nn, 1), np.uint32); score = np.zeros(max(nn, 1), np.int64); pos = np.zeros(max(mem.value, 1), np.int64); end = np.zeros(max(nj, 1), np.int64)
    if self._dll.rv_many_kchain_fetch(self._m, l.ctypes.data, score.ctypes.data, pos.ctypes.data, end.ctypes.data) != 0:
        self._fail()
    return first, l[:nn], score[:nn], pos[:mem.value], end[:nj]


Batch.kchain = _batch_kchain
Batch.kchain_big = _batch_kchain_big
Batch.chains = _batch_chains


class Chains:
    """the chains of `kchain_many`: `arrays` = the CSR (first, l, score, pos, end_score) as numpy arrays; chains[j] = job j's path
    [(l, (p0 .. pk-1), score), ..] in path order, built when asked for; `end_score[j]` = the score of the end sentinel"""

    def __init__(self, arrays, ks):
        self.arrays = arrays
        self.end_score = arrays[4]
        self._k = list(ks)
        first = arrays[0]
        self._poff = np.zeros(len(self._k) + 1, np.int64)      # where each job's positions begin
        np.cumsum((first[1:] - first[:-1]) * np.array(self._k or [0], np.int64)[:len(self._k)], out=self._poff[1:])

    def __len__(self):
        return len(self._k)

    def __getitem__(self, j):
        if not -len(self._k) <= j < len(self._k):
            raise IndexError("job %d of %d" % (j, len(self._k)))
        j %= len(self._k)
        first, l, score, pos, _ = self.arrays
        k, p0 = self._k[j], int(self._poff[j])
        lo, hi = int(first[j]), int(first[j + 1])
        return [(int(l[x]), tuple(int(p) for p in pos[p0 + (x - lo) * k:p0 + (x - lo + 1) * k]), int(score[x])) for x in range(lo, hi)]

    def __iter__(self):
        return (self[j] for j in range(len(self._k)))


def kchain_many(jobs, minlength=20, maxmums=0, wpen=1, wscore=1, gcmodel="sumofpairs", sa64=False, toupper=True, batch=None, large=None):
    """jobs: as for `align_many`.  -> (chains, info): what the reference's `chain()` returns for a fresh index of every job (`offsets` all zero).
    chains: a `Chains`; info = dict(jobs, shared, ordinary, rounds, launches, flagged, big, big_launches): `shared` jobs went through the scan's shared
    launches, `flagged` of them were given back by the kernel; `big` jobs (flagged or ordinary ones) ran the programme in device memory, in
    `big_launches` launches (counted in `launches` too).  `batch`: a Batch to reuse; `large`: sets RV_MANY_SCAN_LARGE as for `mums_many`.  The switches
    (`Batch.option` or the environment): RV_MANY_KCHAIN_HOST chains every job on the host; RV_KCHAIN_CAP lowers the records a job may hold in the
    kernel of the rounds; RV_MANY_KCHAIN_BIG = 0 keeps every list no round has chained on the host; RV_KCHAIN_BIG_MIN: the kept points from which
    such a list goes to the device."""
    if isinstance(jobs, (str, bytes, bytearray)) or not hasattr(jobs, "__iter__"):
        raise error("jobs is a list of jobs")
    if gcmodel not in GCMODELS:
        raise error("unknown gap cost model %r (%s)" % (gcmodel, ", ".join(sorted(GCMODELS))))
    if int(minlength) < 0 or int(maxmums) < 0:
        raise error("minlength >= 0 and maxmums >= 0")
    if not (0 <= int(wpen) <= KCHAIN_WMAX and 0 <= int(wscore) <= KCHAIN_WMAX):
        raise error("weights of 0 .. 2^20")
    prepared = [many.job_sequences(j, toupper) for j in jobs]      # (argument errors before the library is asked for a device)
    b = batch if batch is not None else Batch(sa64)
    if large is not None:
        b.option("RV_MANY_SCAN_LARGE", 1 if large else 0)
    b.clear()
    for seqs in prepared:
        b.add(seqs)
    b.kchain(minlength, maxmums, wpen, wscore, gcmodel)
    info = b.info()
    info["flagged"] = b.flagged().get(KCHAIN_FLAG, 0)
    info["big"], info["big_launches"] = b.kchain_big()
    return Chains(b.chains(), [len(s) for s in prepared]), info


def level_jobs(path_nodes, fromcoord, tocoord, ids, minn):
    """the loop body of chain_cmd (chain.py:78-124) for one chained job: between consecutive path nodes (the begin and the end of the job included),
    each sequence with f + l < t contributes [f + l, t); a gap with at least minn such sequences becomes a job.  path_nodes: [(l, positions)];
    fromcoord / tocoord: the job's begins and ends, all in the coordinates of the top-level sequences; ids: which of them.  -> [(ids', offsets', ends')]"""
    out = []
    f, l = tuple(fromcoord), 0
    for nl, pos in list(path_nodes) + [(0, tuple(tocoord))]:
        sub = [(ids[i], f[i] + l, pos[i]) for i in range(len(ids)) if f[i] + l < pos[i]]
        if any(f[i] + l > pos[i] for i in range(len(ids))):
            raise error("overlapping matches in a chain")
        if len(sub) >= minn:
            out.append(([s[0] for s in sub], [s[1] for s in sub], [s[2] for s in sub]))
        f, l = pos, nl
    return out


def chain_recurse(seqs, minlength=20, minn=2, maxmums=0, wpen=1, wscore=1, gcmodel="sumofpairs", large=True, sa64=False, toupper=True, batch=None):
    """the loop of `reveal chain --recurse` (chain.py:57-124), level by level instead of by a stack: ONE `kchain_many` call per level over all gaps of
    that level (`level_jobs`); a job whose chain is empty ends there.  seqs: the k input sequences, each a sample.  -> (anchors, infos): anchors =
    [(l, ((sequence, position in the top-level text `s0$s1$..`), ..), depth), ..] of all levels, sorted; infos = the `info` of every level's call.  The
    sub-jobs are independent, so the set equals the stack order's.  A top level whose full-match list exceeds the caps of the rounds' kernel runs its
    programme in device memory (`info["big"]`), up to 2^20 full matches.  Not here: the variant nodes, the graph and the GFA of chain_cmd."""
    top = many.job_sequences(seqs, toupper)
    if int(minn) < 2:
        raise error("minn >= 2")
    b = batch if batch is not None else Batch(sa64)
    begin = [sum(len(s) for s in top[:i]) + i for i in range(len(top))]
    level = [(list(range(len(top))), [0] * len(top), [len(s) for s in top])]
    anchors, infos, depth = [], [], 0
    while level:
        jobs = [[top[i][o:e] for i, o, e in zip(ids, offs, ends)] for ids, offs, ends in level]
        chains, info = kchain_many(jobs, minlength, maxmums, wpen, wscore, gcmodel, toupper=False, batch=b, large=large)
        infos.append(info)
        nxt = []
        for (ids, offs, ends), path in zip(level, chains):
            if not path:
                continue
            nodes = [(l, tuple(o + p for o, p in zip(offs, pos))) for l, pos, _ in path]
            anchors += [(l, tuple((i, begin[i] + p) for i, p in zip(ids, pos)), depth) for l, pos in nodes]
            nxt += level_jobs(nodes, offs, ends, ids, int(minn))
        level, depth = nxt, depth + 1
    return sorted(anchors), infos
