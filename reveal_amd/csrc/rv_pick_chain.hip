// rv_pick_chain.hip -- the reference's default picker for the sub-indices of a level of the two-sample level pipeline (k_pick_chain), for rv_many's pair
// jobs above RV_LEAF_N ranks under rv_many_set_picker(1) (RV_MANY_CHAIN_LARGE).
//
// The level pipeline picks on the device: k_pick_slots (rv_scan.hip) writes the longest survivor of the pair scan of every sub-index into picks[1 + s],
// k_decide (rv_decide.hip) turns that into the split's tables.  Under the chain route of rv_many's handle (rv_leaf_chain_route, rv_align.hip) this kernel
// is launched in place of k_pick_slots and writes what schemes.graphmumpicker (reveal/schemes.py:197-361) picks into the same slot: trim the overlaps of
// the sub-index' matches, chain them, split on the largest match of the chain -- the TRIMMED match, which may be shorter than minl.  The decision is
// rv_chain_stage_pair (rv_chain_stage.h); what is here: collecting the scan's survivors, the lists, the flags and writing the pick.  k_decide, the early
// split and the host's bookkeeping stay as they are: to them a pick is a pick.
// Sub-indices whose flag byte says "finished elsewhere" (bit 0: the leaf kernel takes them) are left alone.
//
// What the caller guarantees (rv_many.hip many_class_admits, the RV_MANY_CHAIN_LARGE row of many_classes) is what k_leaf_chain asks for, with other bounds:
//   trim on, minl > 0, no seed possible, a --maxmums that cannot bite, gap model 0 .. 2
//   a job of at most 2^17 ranks          a sub-index' intervals are pieces of its job's two sequences: lengths and positions relative to the interval begins
//                                        lie in [0, 2^17) -- 17 bits each (the kernel flags a job whose interval is longer instead of packing garbage)
//   0 <= wscore, wpen <= RV_LEAF_MCHAIN_WMAX = 2^10
//                                        scores in 32 bits (rv_chain_stage.h): the lengths of a chain (disjoint on path 0) add up to at most 2^17, and a gap
//                                        cost is at most 2^17 (for every model it is bounded by the larger per-path distance, which lies inside the interval +
//                                        the sentinels); a score is at least what the left sentinel offers, gain - wpen * gap >= -2^27, and at most wscore *
//                                        2^17 = 2^27; a candidate score + gain - wpen * gap therefore lies within 3 * 2^27 < 2^30
//
// Packed fields (PairPickStage; the header checks that they fit): a match is l | a << 17 | b << 34, the length field of a sort key has 18 bits (l <= 2^17),
// the sort order in the tie key 16.  The candidate cap must stay below 2^16 - 1; the LDS budget sets it far lower:
//
// Lists in LDS, PC_CAP = 1024 candidates per sub-index: two lists of 8 B and the step numbers of 2 B = 18 B per entry, 18 432 B per workgroup: eight
// workgroups per CU (160 KiB).  At 1 % divergence a pair of 2 x 10 000 bases has about 100 matches of 20 and more bases, a rearranged one a few hundred.
// A sub-index with more candidates flags its job (bit 32) and gets no pick; the job then runs the ordinary way.  RV_PICK_CHAIN_CAP (test hook, in the
// spirit of RV_LEAF_ACAP) lowers the cap so that this is reachable at small shapes.
//
// Shape: ONE wavefront per sub-index, a workgroup of 64 threads.  The chain visits its matches one after the other, each with a reduction over its
// predecessors; inside a wavefront that is two DPP reductions and no barrier.  Several wavefronts per sub-index would put a workgroup barrier and a trip
// through LDS behind every match (up to 1024 of them) to divide work that is a handful of instructions per predecessor, and the sequential cut-back of the
// trim cannot be divided at all; a level holds many sub-indices (one per job at least), so the CUs fill up across sub-indices instead.  The rank sorts
// are quadratic in the candidates (every match counts the ones in front of it): 1024^2 / 64 = 16 384 trips at the cap, three sorts per sub-index.
//
// The flag word is the JOB's: a sub-index of any level belongs to the job whose first sequence holds its interval on path 0 (job_begin: the round's
// ascending text begins, ManyDevJob::abeg).
// No scratch, no VGPR spill (compiler remarks; DESIGN.md 3j quotes them).
#include "rv_scan.h"
#include "rv_chain_stage.h"

namespace {

constexpr int PC_CAP = RV_PICK_CHAIN_CAP_MAX;
static_assert(PC_CAP * 18 <= 160 * 1024 / 8, "eight workgroups per CU");

// the stage's storage (rv_chain_stage.h): the kernel's own LDS lists; positions relative to the sub-index' interval begins, so `left` is -1 on both paths
struct PairPickStage {
    typedef RvMt2 Mt; typedef u64 key_t;
    static constexpr int POS_BITS = 17, CAP = PC_CAP, LMAX = (1 << POS_BITS) - 1, COORD_BITS = POS_BITS, LKEY_BITS = 18, ORDER_BITS = 16;
    u64 *la, *lb; uint16_t *act;
    int aL, bL, aR, bR, wscore, wpen, model;
    __device__ __forceinline__ Mt getA(int i) const { return rv_mt2_unpack<POS_BITS>(la[i]); }
    __device__ __forceinline__ void putA(int i, const Mt &m) { la[i] = rv_mt2_pack<POS_BITS>(m); }
    __device__ __forceinline__ Mt getB(int i) const { return rv_mt2_unpack<POS_BITS>(lb[i]); }
    __device__ __forceinline__ void putB(int i, const Mt &m) { lb[i] = rv_mt2_pack<POS_BITS>(m); }
    __device__ __forceinline__ u64 getE(int i) const { return la[i]; }
    __device__ __forceinline__ void putE(int i, u64 w) { la[i] = w; }
    __device__ __forceinline__ u32 getStep(int i) const { return act[i]; }
    __device__ __forceinline__ void putStep(int i, u32 v) { act[i] = (uint16_t)v; }
    __device__ __forceinline__ int pos(const Mt &m, int c) const { return c ? m.b : m.a; }
    static __device__ __forceinline__ void cut(Mt &m, int overlap) { m.l -= overlap; m.a += overlap; m.b += overlap; }
};

__global__ __launch_bounds__(64) void k_pick_chain(const RvPairRec *__restrict__ slots, const RvPairRec *__restrict__ ovf, u32 ovf_cap,
                                                   const u32 *__restrict__ tilecnt, const u32 *__restrict__ tileovf, int64_t ntile,
                                                   const int64_t *__restrict__ sub_start, int nsubs, RvPairRec *__restrict__ picks,
                                                   u32 *__restrict__ ovf_counter, const u32 *__restrict__ err, RvPickChainArgs P) {
    __shared__ u64 la[PC_CAP];             // list A; during the chain: score (low word) | link << 32
    __shared__ u64 lb[PC_CAP];             // list B
    __shared__ uint16_t act[PC_CAP];       // chain: the step at which a match became active
    const int s = (int)blockIdx.x, lane = (int)threadIdx.x;
    if (s == 0 && lane == 0) {             // the header k_pick_slots writes, and the overflow counter back to zero for the next scan (nothing here reads it)
        u32 *hdr = reinterpret_cast<u32 *>(picks);
        hdr[0] = 0; hdr[1] = *ovf_counter; hdr[2] = err ? *err : 0u; hdr[3] = 0;
        *ovf_counter = 0;
    }
    if (s >= nsubs || (P.flags[s] & 1)) return;                  // finished elsewhere
    const int64_t a0 = (int64_t)P.nodes[4 * (size_t)s], a1 = (int64_t)P.nodes[4 * (size_t)s + 1];
    const int64_t b0 = (int64_t)P.nodes[4 * (size_t)s + 2], b1 = (int64_t)P.nodes[4 * (size_t)s + 3];
    if (!(a0 < a1 && b0 < b1)) return;                           // one sample only: no match, no pick (k_decide decides nothing either)
    const int64_t r0 = sub_start[s], r1 = sub_start[s + 1];
    auto flag_job = [&](u32 bits) { if (lane == 0) atomicOr(&P.job_flags[rv_job_of(P.job_begin, P.njobs, a0)], bits); };
    if (a1 - a0 > PairPickStage::LMAX || b1 - b0 > PairPickStage::LMAX) { flag_job(64u); return; }
    const int cap = (int)(P.cap < (u32)PC_CAP ? P.cap : (u32)PC_CAP);
    PairPickStage t;
    t.la = la; t.lb = lb; t.act = act;

    // ---- collect: the survivors of the pair scan with a rank of this sub-index, in rank order (tiles straddle sub-indices) ----
    int m = 0;
    bool bad = false;
    const int64_t t1 = (r1 - 1) / RV_PAIR_TILE;
    for (int64_t tl = r0 / RV_PAIR_TILE; tl <= t1 && tl < ntile; tl++) {
        const u32 cnt = tilecnt[tl], ob = tileovf[tl];
        for (u32 q0 = 0; q0 < cnt; q0 += 64) {
            const u32 q = q0 + (u32)lane;
            bool ok = false; RvMt2 c; c.l = c.a = c.b = 0;
            if (q < cnt) {
                RvPairRec r; r.a = r.b = 0; r.l = 0; r.rank = 0xFFFFFFFFu;
                if (q < RV_PAIR_SLOTS) r = slots[(size_t)tl * RV_PAIR_SLOTS + q];
                else { const u32 o = ob + (q - RV_PAIR_SLOTS); if (o < ovf_cap) r = ovf[o]; }      // (an overflow list that was too small: the host repeats the scan)
                ok = r.rank != 0xFFFFFFFFu && (int64_t)r.rank >= r0 && (int64_t)r.rank < r1;
                if (ok) {
                    const int64_t ra = (int64_t)r.a, rb = (int64_t)r.b, rl = (int64_t)r.l;
                    if (ra < a0 || ra + rl > a1 || rb < b0 || rb + rl > b1) { ok = false; bad = true; }      // (a match outside the intervals: k_decide's error 4)
                    else { c.l = (int)rl; c.a = (int)(ra - a0); c.b = (int)(rb - b0); }
                }
            }
            const u64 mask = __ballot(ok);
            const int at = m + (int)rv_lanes_below(mask);
            if (ok && at < cap) t.putA(at, c);
            m += (int)__popcll(mask);
        }
    }
    if (__ballot(bad)) { flag_job(2u); return; }
    if (m == 0) return;
    if (m > cap) { flag_job(32u); return; }

    t.aL = -1; t.bL = -1;                                        // `left`: right in front of the intervals
    t.aR = (int)(a1 - a0); t.bR = (int)(b1 - b0);                // `right`: right behind them
    t.wscore = P.wscore; t.wpen = P.wpen; t.model = P.gcmodel;
    RvMt2 pk;
    const int res = rv_chain_stage_pair(t, lane, m, pk);
    if (res > 0) { flag_job((u32)res); return; }
    if (res != RV_STAGE_PICK) return;
    if (lane == 0) { RvPairRec r; r.a = (sa_t)(a0 + pk.a); r.b = (sa_t)(b0 + pk.b); r.l = (u32)pk.l; r.rank = (u32)r0; picks[RV_PAIR_HDR + s] = r; }
}

}  // namespace

int rv_pick_chain_launch(Workspace &ws, const RvPairRec *slots, const RvPairRec *ovf, u32 ovf_cap, const u32 *tilecnt, const u32 *tileovf, int64_t ntile,
                         const int64_t *sub_start, int nsubs, RvPairRec *picks, u32 *ovf_counter, const u32 *err, const RvPickChainArgs &c) {
    if (nsubs <= 0 || !c.nodes || !c.flags || !c.job_flags || !c.job_begin || c.njobs <= 0 || c.wscore < 0 || c.wpen < 0 || c.wscore > RV_PICK_CHAIN_WMAX ||
        c.wpen > RV_PICK_CHAIN_WMAX || c.gcmodel < 0 || c.gcmodel > 2) {
        rv_set_error("rv_pick_chain_launch: arguments the chain pick of the level pipeline does not take");
        return -1;
    }
    hipLaunchKernelGGL(k_pick_chain, dim3((unsigned)nsubs), dim3(64), 0, ws.stream, slots, ovf, ovf_cap, tilecnt, tileovf, ntile, sub_start, nsubs, picks,
                       ovf_counter, err, c);
    RV_LAUNCH_CHECK();
    return 0;
}
