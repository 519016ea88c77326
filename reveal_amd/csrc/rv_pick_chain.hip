// rv_pick_chain.hip -- the reference's default picker for the sub-indices of a level of the two-sample level pipeline (k_pick_chain), for rv_many's pair
// jobs above RV_LEAF_N ranks under rv_many_set_picker(1) (RV_MANY_CHAIN_LARGE).
//
// The level pipeline picks on the device: k_pick_slots (rv_scan.hip) writes the longest survivor of the pair scan of every sub-index into picks[1 + s],
// k_decide (rv_decide.hip) turns that into the split's tables.  Under the chain route of rv_many's handle (rv_leaf_chain_route, rv_align.hip) this kernel
// is launched in place of k_pick_slots and writes what schemes.graphmumpicker (reveal/schemes.py:197-361) picks into the same slot: trim the overlaps of
// the sub-index' matches, chain them, split on the largest match of the chain -- the TRIMMED match, which may be shorter than minl.  rv_pick_chain
// (rv_chain.hip, with pk_trim_overlap of rv_pick.h and rv_chain) is the specification; the stage is PickChain::pick of rv_leaf_chain.hip with wider fields
// and the scan's survivors instead of a scan of its own.  k_decide, the early split and the host's bookkeeping stay as they are: to them a pick is a pick.
// Sub-indices whose flag byte says "finished elsewhere" (bit 0: the leaf kernel takes them) are left alone.
//
// What the caller guarantees (rv_many.hip many_chain_large_admits) is what k_leaf_chain asks for, with other bounds:
//   trim on, minl > 0, no seed possible, a --maxmums that cannot bite, gap model 0 .. 2
//   a job of at most 2^17 ranks          a sub-index' intervals are pieces of its job's two sequences: lengths and positions relative to the interval begins
//                                        lie in [0, 2^17) -- 17 bits each (the kernel flags a job whose interval is longer instead of packing garbage)
//   0 <= wscore, wpen <= RV_LEAF_MCHAIN_WMAX = 2^10
//                                        scores in 32 bits: the lengths of a chain (disjoint on path 0) add up to at most 2^17, and a gap cost is at most 2^17
//                                        (for every model it is bounded by the larger per-path distance, which lies inside the interval + the sentinels); a
//                                        score is at least what the left sentinel offers, gain - wpen * gap >= -2^27, and at most wscore * 2^17 = 2^27; a
//                                        candidate score + gain - wpen * gap therefore lies within 3 * 2^27 < 2^30
//   with weights >= 0 the early `break` of rv_chain never changes the choice (rv_leaf_chain.hip)
//
// Packed fields (all re-derived for 17-bit positions; rv_leaf_chain.hip has 16-bit ones):
//   a match      u64: l (17 bits, 0 .. 16) | a << 17 (17 bits) | b << 34 (17 bits): 51 bits
//   sort key     u64: position << 18 | (2^18 - 1 - l): l <= 2^17 keeps the low field in 18 bits, 35 bits in all; smaller key = in front (position
//                ascending, longer first)
//   chain entry  u64: score (32 bits, two's complement) | link << 32 (16 bits; 0xFFFF = the left sentinel)
//   tie order    k1 (ONE 64-bit key, larger wins) = (candidate score ^ 2^31) << 32 | (predecessor's score ^ 2^31); among equal k1 the smaller
//                k2 = (step of activation + 1) << 16 | sort order (16 + 16 bits; the left sentinel, active from the start: 0)
//   the step at which a match became active: 16 bits, 0xFFFF = not yet
// so the candidate cap must stay below 2^16 - 1; the LDS budget sets it far lower:
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

namespace {

constexpr int PC_CAP = RV_PICK_CHAIN_CAP_MAX;
constexpr u32 LINK_L = 0xFFFFu;        // predecessor: the left sentinel
constexpr u32 NOT_ACTIVE = 0xFFFFu;
constexpr int POS_BITS = 17;
constexpr u64 POS_MASK = (1ull << POS_BITS) - 1;
static_assert(PC_CAP < 0xFFFF, "links, sort order and activation steps are 16-bit fields");
static_assert(PC_CAP * 18 <= 160 * 1024 / 8, "eight workgroups per CU");

#define PC_WSYNC() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier(); } while (0)

struct Mt { int l, a, b; };            // a match: length, position on path 0 / 1 (relative to the sub-index' interval begins)
__device__ inline u64 mt_pack(const Mt &m) { return (u64)(u32)m.l | ((u64)(u32)m.a << POS_BITS) | ((u64)(u32)m.b << (2 * POS_BITS)); }
__device__ inline Mt mt_unpack(u64 w) { Mt m; m.l = (int)(w & POS_MASK); m.a = (int)((w >> POS_BITS) & POS_MASK); m.b = (int)((w >> (2 * POS_BITS)) & POS_MASK); return m; }
__device__ inline u64 sort_key(const Mt &m, int c) { return ((u64)(u32)(c ? m.b : m.a) << 18) | (u64)(262143u - (u32)m.l); }
__device__ inline u32 pc_lanes_below(u64 mask) { return __builtin_amdgcn_mbcnt_hi((u32)(mask >> 32), __builtin_amdgcn_mbcnt_lo((u32)mask, 0u)); }

// utils.gapcost for two paths (rv_chain.hip gapcost): d0, d1 = end of the predecessor - start of the match
__device__ inline int gap2(int d0, int d1, int model) {
    if (model == 1) { const int s = d0 + d1; return (s < 0 ? -s : s) / 2; }
    const int D0 = d0 < 0 ? -d0 : d0, D1 = d1 < 0 ? -d1 : d1;
    if (model == 2) return D0 > D1 ? D0 : D1;
    return D0 > D1 ? D0 - D1 : D1 - D0;
}

// the job whose first sequence holds text position p: the last begin at or in front of it
__device__ inline int job_of(const int64_t *__restrict__ beg, int njobs, int64_t p) {
    int lo = 0, hi = njobs;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (beg[mid] <= p) lo = mid + 1; else hi = mid; }
    return lo > 0 ? lo - 1 : 0;
}

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
    auto flag_job = [&](u32 bits) { if (lane == 0) atomicOr(&P.job_flags[job_of(P.job_begin, P.njobs, a0)], bits); };
    if (a1 - a0 >= ((int64_t)1 << POS_BITS) || b1 - b0 >= ((int64_t)1 << POS_BITS)) { flag_job(64u); return; }
    const int cap = (int)(P.cap < (u32)PC_CAP ? P.cap : (u32)PC_CAP);
    auto getB = [&](int i) { return mt_unpack(lb[i]); };
    auto done = [&](const Mt &m) {
        if (lane == 0) { RvPairRec r; r.a = (sa_t)(a0 + m.a); r.b = (sa_t)(b0 + m.b); r.l = (u32)m.l; r.rank = (u32)r0; picks[RV_PAIR_HDR + s] = r; }
    };

    // ---- collect: the survivors of the pair scan with a rank of this sub-index, in rank order (tiles straddle sub-indices) ----
    int m = 0;
    bool bad = false;
    const int64_t t1 = (r1 - 1) / RV_PAIR_TILE;
    for (int64_t t = r0 / RV_PAIR_TILE; t <= t1 && t < ntile; t++) {
        const u32 cnt = tilecnt[t], ob = tileovf[t];
        for (u32 q0 = 0; q0 < cnt; q0 += 64) {
            const u32 q = q0 + (u32)lane;
            bool ok = false; Mt c; c.l = c.a = c.b = 0;
            if (q < cnt) {
                RvPairRec r; r.a = r.b = 0; r.l = 0; r.rank = 0xFFFFFFFFu;
                if (q < RV_PAIR_SLOTS) r = slots[(size_t)t * RV_PAIR_SLOTS + q];
                else { const u32 o = ob + (q - RV_PAIR_SLOTS); if (o < ovf_cap) r = ovf[o]; }      // (an overflow list that was too small: the host repeats the scan)
                ok = r.rank != 0xFFFFFFFFu && (int64_t)r.rank >= r0 && (int64_t)r.rank < r1;
                if (ok) {
                    const int64_t ra = (int64_t)r.a, rb = (int64_t)r.b, rl = (int64_t)r.l;
                    if (ra < a0 || ra + rl > a1 || rb < b0 || rb + rl > b1) { ok = false; bad = true; }      // (a match outside the intervals: k_decide's error 4)
                    else { c.l = (int)rl; c.a = (int)(ra - a0); c.b = (int)(rb - b0); }
                }
            }
            const u64 mask = __ballot(ok);
            const int at = m + (int)pc_lanes_below(mask);
            if (ok && at < cap) la[at] = mt_pack(c);
            m += (int)__popcll(mask);
        }
    }
    if (__ballot(bad)) { flag_job(2u); return; }
    if (m == 0) return;
    if (m > cap) { flag_job(32u); return; }
    PC_WSYNC();
    if (m == 1) { done(mt_unpack(la[0])); return; }

    // list A -> list B in the stable order of (position on path c, -l): every match counts the ones in front of it
    auto sort_AB = [&](int c, int cnt) {
        for (int base = 0; base < cnt; base += 64) {
            const int i = base + lane;
            Mt me; me.l = me.a = me.b = 0;
            if (i < cnt) me = mt_unpack(la[i]);
            const u64 key = sort_key(me, c);
            int r = 0;
            for (int j = 0; j < cnt; j++) {
                const u64 ko = sort_key(mt_unpack(la[j]), c);      // (the same address for every lane: one broadcast read)
                r += (ko < key || (ko == key && j < i)) ? 1 : 0;
            }
            if (i < cnt) lb[r] = mt_pack(me);
        }
        PC_WSYNC();
    };

    // ---- pk_trim_overlap (rv_pick.h; schemes.py:160-193) ----
    for (int c = 0; c < 2 && m > 1; c++) {
        sort_AB(c, m);
        // the containment filter, B -> A
        const Mt f0 = getB(0), f1 = getB(1);
        const int end0 = (c ? f0.b : f0.a) + f0.l, end1 = (c ? f1.b : f1.a) + f1.l;
        int w = 0;
        for (int base = 0; base < m; base += 64) {
            const int i = base + lane;
            bool keep = false; Mt me; me.l = me.a = me.b = 0;
            if (i < m) {
                me = getB(i);
                const Mt pv = getB(i == 0 ? m - 1 : i - 1);      // (i - 1 == -1: the last one)
                const int en = (c ? me.b : me.a) + me.l, ep = (c ? pv.b : pv.a) + pv.l;
                keep = (i == 0 && end1 > end0) || ep < en;
            }
            const u64 mask = __ballot(keep);
            if (keep) la[w + (int)pc_lanes_below(mask)] = mt_pack(me);
            w += (int)__popcll(mask);
        }
        m = w;
        PC_WSYNC();
        if (m <= 1) break;
        // the cut-back: `trimmed` is the stack la[0 .. top], written in place (it never holds more than the i matches read so far).  Every lane
        // follows the same values (broadcast reads), lane 0 writes.
        int top = 0;
        bool raised = false;
        for (int i = 1; i < m; i++) {
            if (top < 0) { raised = true; break; }            // trimmed[-1] of an empty list: the reference raises IndexError
            const Mt mum = mt_unpack(la[i]);
            Mt pm = mt_unpack(la[top]);
            const int overlap = (c ? pm.b : pm.a) + pm.l - (c ? mum.b : mum.a);
            if (overlap > 0) {
                if (pm.l - overlap > 0) { pm.l -= overlap; if (lane == 0) la[top] = mt_pack(pm); }
                else top--;
                if (mum.l - overlap > 0) {
                    Mt t = mum; t.l -= overlap; t.a += overlap; t.b += overlap;
                    top++;
                    if (lane == 0) la[top] = mt_pack(t);
                }
            } else {
                top++;
                if (lane == 0) la[top] = mt_pack(mum);
            }
            PC_WSYNC();
        }
        if (raised) { flag_job(1u); return; }
        m = top + 1;
    }
    if (m == 0) return;
    if (m == 1) { done(mt_unpack(la[0])); return; }

    // ---- rv_chain for two paths ----
    sort_AB(0, m);                                          // the order of path 0 (distinct coordinates)
    for (int i = lane; i < m; i += 64) act[i] = (uint16_t)NOT_ACTIVE;
    PC_WSYNC();
    const int aL = -1, bL = -1;                             // `left`: right in front of the intervals
    const int aR = (int)(a1 - a0), bR = (int)(b1 - b0);     // `right`: right behind them
    const int wscore = P.wscore, wpen = P.wpen, model = P.gcmodel;
    u32 linkR = LINK_L;
    for (int e = 0; e <= m; e++) {
        Mt me; me.l = 0; me.a = aR; me.b = bR;
        if (e < m) me = getB(e);
        const int gain = wscore * me.l;                     // n (n - 1) / 2 = 1 for two members; `right` has none
        u64 b1k = 0; u32 b2k = 0xFFFFFFFFu;
        if (lane == 0 && aL <= me.a && bL <= me.b) {
            const int tmpw = gain - wpen * gap2(aL - me.a, bL - me.b, model);
            b1k = ((u64)((u32)tmpw ^ 0x80000000u) << 32) | (u64)(0u ^ 0x80000000u);
            b2k = 0;
        }
        for (int base = 0; base < e; base += 64) {
            const int p = base + lane;
            if (p < e) {
                const Mt o = getB(p);
                if (o.a + o.l <= me.a && o.b + o.l <= me.b) {      // ends at or in front of the match on both paths
                    u32 st = act[p];
                    if (st == NOT_ACTIVE) { st = (u32)e; act[p] = (uint16_t)e; }
                    const int sc = (int)(u32)(la[p] & 0xFFFFFFFFull);
                    const int tmpw = sc + gain - wpen * gap2(o.a + o.l - me.a, o.b + o.l - me.b, model);
                    const u64 k1 = ((u64)((u32)tmpw ^ 0x80000000u) << 32) | (u64)((u32)sc ^ 0x80000000u);
                    const u32 k2 = ((st + 1u) << 16) | (u32)p;
                    if (k1 > b1k || (k1 == b1k && k2 < b2k)) { b1k = k1; b2k = k2; }
                }
            }
        }
        const u64 w1 = rv_wave_max_u64(b1k);
        if (w1 == 0) { flag_job(2u); return; }              // (a match that does not lie behind `left`: rv_chain fails)
        const u32 w2 = 0xFFFFFFFFu - (u32)rv_wave_max_u64((u64)(0xFFFFFFFFu - (b1k == w1 ? b2k : 0xFFFFFFFFu)));
        const u32 link = w2 < 65536u ? LINK_L : (w2 & 0xFFFFu);
        const u32 score = (u32)(w1 >> 32) ^ 0x80000000u;
        if (e < m) { if (lane == 0) la[e] = (u64)score | ((u64)link << 32); }
        else linkR = link;
        PC_WSYNC();
    }
    // back from `right`: the largest of the chain, of equal lengths the last in chain order = the first met on the way back
    int split = -1, bl = 0, guard = 0;
    for (u32 c = linkR; c != LINK_L; c = (u32)(la[c] >> 32) & 0xFFFFu) {
        if (c >= (u32)m || ++guard > m) { flag_job(2u); return; }      // (broken back-pointer chain)
        const int l = getB((int)c).l;
        if (l > bl) { bl = l; split = (int)c; }
    }
    if (split < 0) return;                                  // `right` links to `left`: an empty chain, nothing picked
    done(getB(split));
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
