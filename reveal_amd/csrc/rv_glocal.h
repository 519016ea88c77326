// rv_glocal.h -- the glocal chain of `reveal transform` (transform.py:301-360, glocalchain :947-1180 with useheap=False, gapcost :1182-1244):
// rv_glocal.hip.  The rule is stated in include/reveal_amd.h (rv_glocal_filter); the cost of an edge is ONE function below, compiled for the host
// rule and for the kernels alike.
#pragma once
#include "rv_common.h"
#include <vector>

struct RvGlcParams { int64_t rearr, inv, lambda, eps, alfa, gapopen, lastn, lastbp; };      // the order of the ABI's params[8]

// the caller's list and the sequences' ranges, all on the host
struct RvGlcIn {
    int64_t n = 0;
    const int64_t *s1 = nullptr, *e1 = nullptr, *s2 = nullptr, *e2 = nullptr; const int32_t *o = nullptr; const int64_t *score = nullptr;
    const int32_t *refid = nullptr, *ctgid = nullptr;
    int64_t nseq = 0; const int64_t *rs = nullptr, *re = nullptr;      // (begin, '$') of every sequence in order of addition
    int64_t sep = 0;                                                  // sequences that begin in front of it are the reference's
};
struct RvGlcOut {
    std::vector<int32_t> idx;      // the chain: indices into the caller's list, in chain order
    void clear() { idx.clear(); }
};
// info[] of a call (int64): the first RV_GLC_INFO_HEAD words, then the blocks left by every pass as far as the array reaches
enum { RV_GLC_ROUTE = 0, RV_GLC_PASSES0, RV_GLC_PASSES1, RV_GLC_TILES, RV_GLC_TILES_MAX, RV_GLC_CHAIN_NS, RV_GLC_CHAIN_BLOCKS, RV_GLC_BYTES_UP, RV_GLC_BYTES_DOWN,
       RV_GLC_EDGES, RV_GLC_SORT_KEYS, RV_GLC_NAFTER, RV_GLC_INFO_HEAD };

// an entry of a pass in the coordinates of its axis: [a, ae] on the axis the pass sorts by, [b, be] on the other one; id1 / id2 = the sequences it
// lies in on the two axes, id1 < 0 for a dummy (a sequence end, or `start`)
struct GlcEntry { int64_t a, ae, b, be; int32_t o, id1, id2; };

// gapcost (transform.py:1182-1244) of two entries inside one reference sequence and one contig, 1 in front of 2
__host__ __device__ inline int64_t glc_gapcost(int64_t ae1, int64_t b1, int64_t be1, int o1, int64_t a2, int64_t b2, int64_t be2, int o2, const RvGlcParams &w) {
    int64_t d1 = a2 - ae1, d2, inv = 0;
    if (o1 == o2) {
        const bool fwd = o1 == 0;
        if (fwd ? (b2 < b1) : (b2 > b1)) return w.gapopen + w.rearr + w.eps * (d1 > 0 ? d1 : 0);      // against the orientation: always a rearrangement
        d2 = fwd ? b2 - be1 : b1 - be2;
    } else {
        if (d1 < 0) d1 = 0;
        d2 = b2 > b1 ? b2 - be1 : b1 - be2;
        if (d2 < 0) d2 = 0;
        inv = w.inv;
    }
    int64_t diff = d1 - d2;
    if (diff < 0) diff = -diff;
    int64_t indel = w.lambda * diff;
    if (indel > w.rearr) indel = w.rearr;
    int64_t sub = d1 < d2 ? d1 : d2;
    if (sub < 0) sub = 0;
    return w.gapopen + indel + w.eps * sub + inv;
}
__host__ __device__ inline int64_t glc_abs(int64_t x) { return x < 0 ? -x : x; }
// what the step from predecessor p to block b costs (transform.py:1070-1127); rs / re = the sequences' ranges
__host__ __device__ inline int64_t glc_cost(const GlcEntry &p, const GlcEntry &b, int axis, const RvGlcParams &w, const int64_t *rs, const int64_t *re) {
    if (p.id1 < 0 && b.id1 < 0) return w.gapopen + glc_abs(b.a - p.ae) * w.eps;
    if (b.id1 < 0) {                 // the dummy made relative to its predecessor: same sequences, same orientation, at the point where p ends
        const int64_t x = p.o == 0 ? p.be : p.b;
        return glc_gapcost(p.ae, p.b, p.be, p.o, b.a, x, x, p.o, w);
    }
    if (p.id1 < 0) {                 // ... and a dummy predecessor at the point where b begins
        const int64_t y = b.o == 0 ? b.b : b.be;
        return glc_gapcost(p.ae, y, y, b.o, b.a, b.b, b.be, b.o, w);
    }
    if (p.id1 == b.id1 && p.id2 == b.id2) return glc_gapcost(p.ae, p.b, p.be, p.o, b.a, b.b, b.be, b.o, w);
    if (p.id1 == b.id1) {            // same sequence on the sorted axis, another one on the other axis: what is left of both to their sequences' ends
        const int64_t cp = p.o == 0 ? glc_abs(re[p.id2] - p.be) : glc_abs(p.b - rs[p.id2]);
        const int64_t cb = ((b.o == 0) == (axis == 0)) ? glc_abs(re[b.id2] - b.be) : glc_abs(b.b - rs[b.id2]);
        const int64_t c = (cp + cb) * w.eps;
        return w.gapopen + (c < w.rearr ? c : w.rearr);
    }
    return w.rearr + w.gapopen + glc_abs(b.a - p.ae) * w.eps;
}
// the two filters (transform.py:1052-1056): a predecessor that does not lie in front of b on the sorted axis, or lies inside b on the other one
__host__ __device__ inline bool glc_skip(int64_t pa, int64_t pae, int64_t pb, int64_t pbe, int32_t pid1, int64_t ba, int64_t bae, int64_t bb, int64_t bbe, int32_t bid1) {
    if (pid1 < 0 || bid1 < 0) return false;
    return pa == ba || pae >= bae || (pb >= bb && pbe <= bbe);
}

// 1: these weights on a list of n blocks (coordinates <= maxcoord, scores <= maxscore) stay inside 62 bits; 0: they might not; -1: a negative weight
int rv_glocal_admit_rule(int64_t n, int64_t nseq, int64_t maxcoord, int64_t maxscore, const RvGlcParams &w);
// the list's own consistency (s <= e, ids, orientation, non-negative scores and coordinates); -> 0, the two maxima filled in
int rv_glocal_validate(const RvGlcIn &in, int64_t *maxcoord, int64_t *maxscore);
// axes: bit 0 the reference axis, bit 1 the query axis; fixed = 0: one pass per axis named, 1: every axis to its fixed point (transform.py:307-356)
int rv_glocal_rule_host(const RvGlcIn &in, const RvGlcParams &w, int axes, int fixed, int64_t *info, int ninfo, RvGlcOut &out);
int rv_glocal_device(Workspace &ws, const RvGlcIn &in, const RvGlcParams &w, int axes, int fixed, int64_t *info, int ninfo, RvGlcOut &out);
