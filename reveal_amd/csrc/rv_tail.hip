// rv_tail.hip -- chainscore (transform.py:836-935) and one sweep of optimise (:801-834) in host C++; the rules are stated in include/reveal_amd.h
// (rv_chainscore_host, rv_optimise_host).
//
// The reference's sweep scores the chain once per candidate and sorts it twice each time: quadratic with a sort inside.  Here the two orders are
// made once -- the reference order (s1, ties as the reference's stable sort leaves them) and the query order (s2, ties in reference order) -- and kept
// as doubly linked lists.  Leaving a block out is unlinking it from both; a block's neighbours in the query order, which is all chainscore asks of
// the ranks, are its links.  A candidate costs one walk along the reference list.
#include "rv_tail.h"
#include <algorithm>
#include <numeric>

namespace {

// both orders over the rows of a list; tie[i] decides between rows of equal s1
struct TailOrder {
    std::vector<int32_t> nextr, prevr, nextq, prevq;
    int32_t headr = -1, tailr = -1;
    void build(const RvTailIn &in, const std::vector<int32_t> &tie) {
        const size_t n = (size_t)in.n;
        std::vector<int32_t> byref(n), byq(n), refpos(n);
        std::iota(byref.begin(), byref.end(), 0);
        std::sort(byref.begin(), byref.end(), [&](int32_t x, int32_t y) { return in.s1[x] != in.s1[y] ? in.s1[x] < in.s1[y] : tie[(size_t)x] < tie[(size_t)y]; });
        for (size_t k = 0; k < n; k++) refpos[(size_t)byref[k]] = (int32_t)k;
        byq = byref;
        std::sort(byq.begin(), byq.end(), [&](int32_t x, int32_t y) { return in.s2[x] != in.s2[y] ? in.s2[x] < in.s2[y] : refpos[(size_t)x] < refpos[(size_t)y]; });
        nextr.assign(n, -1); prevr.assign(n, -1); nextq.assign(n, -1); prevq.assign(n, -1);
        for (size_t k = 0; k + 1 < n; k++) {
            nextr[(size_t)byref[k]] = byref[k + 1]; prevr[(size_t)byref[k + 1]] = byref[k];
            nextq[(size_t)byq[k]] = byq[k + 1]; prevq[(size_t)byq[k + 1]] = byq[k];
        }
        headr = n ? byref[0] : -1; tailr = n ? byref[n - 1] : -1;
    }
    void unlink(int32_t c) {
        const int32_t pr = prevr[(size_t)c], nr = nextr[(size_t)c], pq = prevq[(size_t)c], nq = nextq[(size_t)c];
        if (pr >= 0) nextr[(size_t)pr] = nr; else headr = nr;
        if (nr >= 0) prevr[(size_t)nr] = pr; else tailr = pr;
        if (pq >= 0) nextq[(size_t)pq] = nq;
        if (nq >= 0) prevq[(size_t)nq] = pq;
    }
    void relink(int32_t c) {      // (undoes the unlink made last)
        const int32_t pr = prevr[(size_t)c], nr = nextr[(size_t)c], pq = prevq[(size_t)c], nq = nextq[(size_t)c];
        if (pr >= 0) nextr[(size_t)pr] = c; else headr = c;
        if (nr >= 0) prevr[(size_t)nr] = c; else tailr = c;
        if (pq >= 0) nextq[(size_t)pq] = c;
        if (nq >= 0) prevq[(size_t)nq] = c;
    }
};

// chainscore of the rows linked in T
int tail_score(const RvTailIn &in, const RvGlcParams &w, const TailOrder &T, int64_t *weight, int64_t *cost, std::vector<int64_t> *edges) {
    if (edges) edges->clear();
    const int64_t rl = in.rlength, ql = in.qlength;
    if (T.headr < 0) {
        const int64_t c = glc_gapcost(0, rl, rl, 0, rl, rl + ql, rl + ql, 0, w);
        *weight = 0; *cost = c;
        if (edges) edges->push_back(c);
        return 0;
    }
    const int32_t first = T.headr, last = T.tailr;
    const int32_t o0 = in.o[first];
    const int64_t sq = o0 == 0 ? in.rs[in.ctgid[first]] : in.re[in.ctgid[first]];      // `start` and `end` both take the first block's orientation
    const int64_t eq = o0 == 0 ? in.re[in.ctgid[last]] : in.rs[in.ctgid[last]];
    if (in.s1[last] > rl) { rv_set_error("chainscore: a block begins behind rlength"); return -1; }
    int64_t c = glc_gapcost(0, sq, sq, o0, in.s1[first], in.s2[first], in.e2[first], in.o[first], w);
    int64_t total = c, wt = w.alfa * in.score[first];
    if (edges) edges->push_back(c);
    const int64_t rearr = w.gapopen + w.rearr;
    for (int32_t p = first, b = T.nextr[(size_t)first]; b >= 0; p = b, b = T.nextr[(size_t)b]) {
        wt += w.alfa * in.score[b];
        if (in.ctgid[p] == in.ctgid[b] && in.refid[p] == in.refid[b]) {
            if (T.nextq[(size_t)p] == b || T.prevq[(size_t)p] == b) c = glc_gapcost(in.e1[p], in.s2[p], in.e2[p], in.o[p], in.s1[b], in.s2[b], in.e2[b], in.o[b], w);      // collinear
            else c = rearr;
            total += c;
        } else {
            // another block of either contig lies between the two in the query order: a rearrangement; otherwise a plain step to the next contig,
            // which enters the edge costs and not the cost (as the reference has it)
            const int32_t pq = in.o[b] == 0 ? T.prevq[(size_t)b] : T.nextq[(size_t)b];
            const int32_t nq = in.o[p] == 0 ? T.nextq[(size_t)p] : T.prevq[(size_t)p];
            if ((pq >= 0 && in.ctgid[pq] == in.ctgid[b]) || (nq >= 0 && in.ctgid[nq] == in.ctgid[p])) { c = rearr; total += c; }
            else c = w.gapopen;
        }
        if (edges) edges->push_back(c);
    }
    c = glc_gapcost(in.e1[last], in.s2[last], in.e2[last], in.o[last], rl, eq, eq, o0, w);
    total += c;
    if (edges) edges->push_back(c);
    *weight = wt; *cost = total;
    return 0;
}

}  // namespace

int rv_tail_validate(const RvTailIn &in, const RvGlcParams &w) {
    if (in.n < 0 || in.nseq < 0 || (in.nseq && (!in.rs || !in.re)) || (in.n && (!in.s1 || !in.e1 || !in.s2 || !in.e2 || !in.o || !in.score || !in.refid || !in.ctgid))) {
        rv_set_error("chainscore: bad arguments"); return -1;
    }
    if (in.n > 0x7ffffff0ll) { rv_set_error("chainscore: more than 2^31 - 16 blocks"); return -1; }
    const int64_t lim = (int64_t)1 << 61;
    if (in.rlength < 0 || in.qlength < 0 || in.rlength >= lim || in.qlength >= lim || in.rlength + in.qlength >= lim) { rv_set_error("chainscore: rlength / qlength outside 0 .. 2^61"); return -1; }
    int64_t mc = in.rlength + in.qlength, ms = 0;
    for (int64_t i = 0; i < in.nseq; i++) {
        if (in.rs[i] < 0 || in.re[i] < 0 || in.rs[i] >= lim || in.re[i] >= lim) { rv_set_error("chainscore: ctg2range outside 0 .. 2^61"); return -1; }
        mc = std::max(mc, std::max(in.rs[i], in.re[i]));
    }
    for (int64_t i = 0; i < in.n; i++) {
        if (in.s1[i] < 0 || in.e1[i] < 0 || in.s2[i] < 0 || in.e2[i] < 0 || in.s1[i] >= lim || in.e1[i] >= lim || in.s2[i] >= lim || in.e2[i] >= lim) {
            rv_set_error("chainscore: block %lld: coordinates outside 0 .. 2^61", (long long)i); return -1;
        }
        if (in.o[i] != 0 && in.o[i] != 1) { rv_set_error("chainscore: block %lld: orientation is 0 or 1", (long long)i); return -1; }
        if (in.score[i] < 0 || in.score[i] >= lim) { rv_set_error("chainscore: block %lld: score outside 0 .. 2^61", (long long)i); return -1; }
        if (in.ctgid[i] < 0 || in.ctgid[i] >= in.nseq) { rv_set_error("chainscore: block %lld: ctgid names no sequence", (long long)i); return -1; }
        mc = std::max(mc, std::max(std::max(in.s1[i], in.e1[i]), std::max(in.s2[i], in.e2[i]))); ms = std::max(ms, in.score[i]);
    }
    const int r = rv_glocal_admit_rule(in.n, in.nseq, mc, ms, w);
    if (r < 0) return -1;
    if (r == 0) { rv_set_error("chainscore: these weights are outside the library's integer arithmetic"); return -1; }
    return 0;
}

int rv_chainscore_rule_host(const RvTailIn &in, const RvGlcParams &w, int64_t *weight, int64_t *cost, std::vector<int64_t> *edgecosts) {
    try {
        std::vector<int32_t> tie((size_t)in.n);
        std::iota(tie.begin(), tie.end(), 0);
        TailOrder T;
        T.build(in, tie);
        return tail_score(in, w, T, weight, cost, edgecosts);
    } catch (...) { rv_set_error("chainscore: out of host memory"); return -1; }
}

int rv_optimise_rule_host(const RvTailIn &in, const RvGlcParams &w, int64_t *weight, int64_t *cost, std::vector<int32_t> &kept) {
    kept.clear();
    try {
        const size_t n = (size_t)in.n;
        std::vector<int32_t> tie(n), org(n);
        std::iota(tie.begin(), tie.end(), 0);
        TailOrder T0;                    // the chain as it comes: ties of s1 in list order
        T0.build(in, tie);
        int64_t bw = 0, bc = 0;
        if (tail_score(in, w, T0, &bw, &bc, nullptr) != 0) return -1;
        // the candidates in ascending score, ties in list order; the chains they are left out of hold the others in this order
        std::iota(org.begin(), org.end(), 0);
        std::stable_sort(org.begin(), org.end(), [&](int32_t x, int32_t y) { return in.score[x] < in.score[y]; });
        for (size_t k = 0; k < n; k++) tie[(size_t)org[k]] = (int32_t)k;
        TailOrder T;
        T.build(in, tie);
        bool dropped = false;
        for (size_t k = 0; k < n; k++) {
            const int32_t c = org[k];
            T.unlink(c);
            int64_t tw = 0, tc = 0;
            if (tail_score(in, w, T, &tw, &tc, nullptr) != 0) return -1;
            if (tw - tc < bw - bc) T.relink(c);      // the chain is worse without it: it stays
            else { bw = tw; bc = tc; dropped = true; }
        }
        const TailOrder &R = dropped ? T : T0;
        for (int32_t b = R.headr; b >= 0; b = R.nextr[(size_t)b]) kept.push_back(b);
        *weight = bw; *cost = bc;
    } catch (...) { rv_set_error("optimise: out of host memory"); return -1; }
    return 0;
}
