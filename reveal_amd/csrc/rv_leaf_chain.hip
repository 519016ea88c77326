// rv_leaf_chain.hip -- the leaf kernel with the reference's default picker as its pick stage (k_leaf_chain), for rv_many's pair jobs: the whole job where it has at
// most RV_LEAF_N ranks (RV_MANY_CHAIN), and the sub-indices of larger jobs once they are leaf-sized (RV_MANY_CHAIN_LARGE; the picks above are rv_pick_chain.hip's).
//
// `reveal refine --method reveal_rem` aligns a bubble with schemes.graphmumpicker (reveal/schemes.py:197-361): trim the overlaps of the sub-index'
// matches, chain them, split on the largest match of the chain.  That decision for TWO samples is rv_chain_stage_pair (rv_chain_stage.h), made by the
// wavefront that owns the sub-index, so a job's whole recursion stays in one workgroup as it does with the built-in picker.  Frame stack, split,
// bubble_sort and anchor staging are k_leaf's (rv_leaf_stages.h: leaf_run).  What is here: collect, where the lists live, what happens to a pick.
//
// What the caller guarantees (rv_many.hip many_class_admits, the RV_MANY_CHAIN row of many_classes), and what follows from it:
//   trim on, minl > 0          no p-value cut (pow / exp / log stay on the host)
//   no seed can arise          the "precomputed" branch of the picker is never needed: a child starts from its scan like the root
//   --maxmums cannot bite      two MUMs never start at the same position of either sequence: a sub-index holds at most min(la, lb) of them
//   0 <= wscore, wpen <= RV_LEAF_CHAIN_WMAX = 2^16
//                              scores in 32 bits (rv_chain_stage.h): a job has at most 2^11 ranks, so every gap cost is at most 2^11 and the lengths of a
//                              chain (disjoint on path 0) add up to at most 2^11; a score is at least what the left sentinel offers, gain - wpen * gap >=
//                              -2^27, and at most wscore * 2^11 = 2^27; a candidate score + gain - wpen * gap lies within 3 * 2^27 < 2^30
//
// collect   every candidate of the scan predicate (reveal.c:131-159) of a sub-index of `len` ranks, in rank order, as (l, a, b), positions relative to
//           the job's sequences (16 bits each).  Fewer than `len` candidates; the lists are indexed from the sub-index' first rank, as act[] is: the
//           waves of a workgroup own disjoint rank ranges, so nothing overflows or collides and nothing depends on the job's shape.
//
// LDS: k_leaf's 50 424 B (32-bit suffix arrays; 68 856 B with 64-bit ones) + one list of 8 B per rank = 16 KB.  The second list of the sorts and
// the step numbers of the chain live in the ranks [S, E) of the OTHER copy of the sub-index' arrays and of act[], which are free until the split
// writes the children there (the live frames of a root have disjoint rank ranges).  66 808 B: two workgroups per CU (k_leaf: three); the 64-bit
// library 85 240 B: one.  160 KiB per CU.  No scratch (compiler remarks; DESIGN.md 3j quotes them).
#include "rv_leaf_stages.h"
#include "rv_chain_stage.h"

namespace {

// the flag word of the root's JOB (the cold path: a root that cannot be finished).  The roots of a launch are whole jobs in a small round and sub-indices of
// jobs, at any level, in a large one: the host ships the job of every root with the launch (found among the round's text begins, rv_align.hip leaf_launch).
// (Searched here instead, inlined, the begins cost a VGPR and seven spilled SGPRs; out of line, 48 B of scratch.)
__device__ inline u32 *job_flag(const RvLeafChainArgs &P) { return P.flags + P.root_job[blockIdx.x]; }

// the stage's storage (rv_chain_stage.h): list A and the chain entries in eA, list B split over the other copy's LCP words (l | a << 16) and suffix
// words (b; sa_t: the two libraries differ), the steps in act[] -- all from the sub-index' first rank
struct PairLeafStage {
    typedef RvMt2 Mt; typedef u32 key_t;
    static constexpr int CAP = LN, LMAX = LN, POS_BITS = 16, COORD_BITS = POS_BITS, LKEY_BITS = 12, ORDER_BITS = 12;
    u64 *la; u32 *lb_la; sa_t *lb_b; uint16_t *act;
    int aL, bL, aR, bR, wscore, wpen, model;
    __device__ __forceinline__ Mt getA(int i) const { return rv_mt2_unpack<POS_BITS>(la[i]); }
    __device__ __forceinline__ void putA(int i, const Mt &m) { la[i] = rv_mt2_pack<POS_BITS>(m); }
    __device__ __forceinline__ Mt getB(int i) const { Mt m; const u32 w = lb_la[i]; m.l = (int)(w & 0xFFFFu); m.a = (int)(w >> 16); m.b = (int)lb_b[i]; return m; }
    __device__ __forceinline__ void putB(int i, const Mt &m) { lb_la[i] = (u32)m.l | ((u32)m.a << 16); lb_b[i] = (sa_t)m.b; }
    __device__ __forceinline__ u64 getE(int i) const { return la[i]; }
    __device__ __forceinline__ void putE(int i, u64 w) { la[i] = w; }
    __device__ __forceinline__ u32 getStep(int i) const { return act[i]; }
    __device__ __forceinline__ void putStep(int i, u32 v) { act[i] = (uint16_t)v; }
    __device__ __forceinline__ int pos(const Mt &m, int c) const { return c ? m.b : m.a; }
    static __device__ __forceinline__ void cut(Mt &m, int overlap) { m.l -= overlap; m.a += overlap; m.b += overlap; }
};

struct PickChain {
    static __device__ __forceinline__ void fail(const RvLeafArgs &, const RvLeafChainArgs &P, u32 bits) { atomicOr(job_flag(P), bits); }

    static __device__ __forceinline__ bool pick(const RvLeafArgs &, const RvLeafChainArgs &P, const LeafSub &X, u32 &L, int64_t &pa, int64_t &pb) {
        __shared__ u64 eA[LN];
        const int S = X.S, E = X.E, lane = X.lane;
        PairLeafStage t;
        t.la = eA + S; t.lb_la = X.nl + S; t.lb_b = X.ns + S; t.act = X.act + S;
        const sa_t nsep0 = X.nsep0;

        // ---- collect: the candidates of the scan predicate, in rank order ----------------------------------------------
        int m = 0;
        for (int base = S; base < E; base += 64) {
            const int i = base + lane;
            bool ok = false; RvMt2 c; c.l = c.a = c.b = 0;
            if (i < E && i > S) {
                const u32 l = X.cl[i]; const sa_t s1 = X.cs[i], s0 = X.cs[i - 1];
                const u32 nx = (i + 1 < E) ? X.cl[i + 1] : 0u;
                ok = l >= X.minl && ((s1 > nsep0) != (s0 > nsep0)) && X.cl[i - 1] < l && nx < l &&
                     (s1 < s0 ? left_maximal(X.cb[i], X.cb[i - 1]) : left_maximal(X.cb[i - 1], X.cb[i]));
                c.l = (int)l; c.a = (int)((int64_t)(s1 < s0 ? s1 : s0) - X.ra0); c.b = (int)((int64_t)(s1 < s0 ? s0 : s1) - X.rb0);
            }
            const u64 mask = __ballot(ok);
            if (ok) t.putA(m + (int)rv_lanes_below(mask), c);
            m += (int)__popcll(mask);
        }
        if (!X.both || m == 0) return false;
        t.aL = (int)(X.f.a0 - 1 - X.ra0); t.bL = (int)(X.f.b0 - 1 - X.rb0);      // `left`: right in front of the intervals
        t.aR = (int)(X.f.a1 - X.ra0); t.bR = (int)(X.f.b1 - X.rb0);              // `right`: right behind them
        t.wscore = P.wscore; t.wpen = P.wpen; t.model = P.gcmodel;
        RvMt2 pk;
        const int r = rv_chain_stage_pair(t, lane, m, pk);
        if (r > 0 && lane == 0) atomicOr(job_flag(P), (u32)r);      // (the job finishes on the host)
        if (r != RV_STAGE_PICK) return false;
        L = (u32)pk.l; pa = X.ra0 + pk.a; pb = X.rb0 + pk.b;      // the anchor is the TRIMMED match
        return true;
    }
};

__global__ __launch_bounds__(NT) void k_leaf_chain(RvLeafArgs A, RvLeafChainArgs C) { leaf_run<PickChain>(A, C); }

}  // namespace

int rv_leaf_chain_launch(Workspace &ws, const RvLeafArgs &a, const RvLeafChainArgs &c, int nroots) {
    if (nroots <= 0) return 0;
    if (a.trace || !c.flags || !c.root_job || c.wscore < 0 || c.wpen < 0 || c.wscore > RV_LEAF_CHAIN_WMAX || c.wpen > RV_LEAF_CHAIN_WMAX || c.gcmodel < 0 || c.gcmodel > 2) {
        rv_set_error("rv_leaf_chain_launch: arguments the chain form of the leaf kernel does not take");
        return -1;
    }
    hipLaunchKernelGGL(k_leaf_chain, dim3((unsigned)nroots), dim3(NT), 0, ws.stream, a, c);
    RV_LAUNCH_CHECK();
    return 0;
}
