// rv_leaf_chain.hip -- the leaf kernel with the reference's default picker as its pick stage (k_leaf_chain), for rv_many's pair jobs: the whole job where it has at
// most RV_LEAF_N ranks (RV_MANY_CHAIN), and the sub-indices of larger jobs once they are leaf-sized (RV_MANY_CHAIN_LARGE; the picks above are rv_pick_chain.hip's).
//
// `reveal refine --method reveal_rem` aligns a bubble with schemes.graphmumpicker (reveal/schemes.py:197-361): trim the overlaps of the sub-index'
// matches, chain them, split on the largest match of the chain.  rv_pick_chain (rv_chain.hip, with pk_trim_overlap of rv_pick.h and rv_chain) is that
// picker in host C++ and the specification of this stage; here its decision for TWO samples is made by the wavefront that owns the sub-index, so a
// job's whole recursion stays in one workgroup as it does with the built-in picker.  Frame stack, split, bubble_sort and anchor staging are k_leaf's
// (rv_leaf_stages.h: leaf_run).
//
// What the caller guarantees (rv_many.hip many_chain_admits), and what follows from it:
//   trim on, minl > 0          no p-value cut (pow / exp / log stay on the host)
//   no seed can arise          the "precomputed" branch of the picker is never needed: a child starts from its scan like the root
//   --maxmums cannot bite      two MUMs never start at the same position of either sequence: a sub-index holds at most min(la, lb) of them
//   0 <= wscore, wpen <= RV_LEAF_CHAIN_WMAX = 2^16
//                              scores in 32 bits: a job has at most 2^11 ranks, so every gap cost is at most 2^11 and the lengths of a chain (disjoint on
//                              path 0) add up to at most 2^11; a score is at least what the left sentinel offers, gain - wpen * gap >= -2^27, and at most
//                              wscore * 2^11 = 2^27; a candidate score + gain - wpen * gap lies within 3 * 2^27 < 2^30
//   with weights >= 0 the early `break` of rv_chain never changes the choice (a later predecessor's score + gain is already below the best found)
//
// The stage, for a sub-index of `len` ranks (fewer than `len` candidates; lists indexed from the sub-index' first rank, as act[] is: the waves of a
// workgroup own disjoint rank ranges, so nothing overflows or collides and nothing depends on the job's shape):
//   collect   every candidate of the scan predicate (reveal.c:131-159) in rank order -- the order pick_one (rv_align.hip) hands records to
//             rv_pick_chain -- as (l, a, b), positions relative to the job's sequences (16 bits each)
//   trim      pk_trim_overlap on path 0, then path 1: stable rank sort by (position, -l), the containment filter (the element in front of the
//             first is the LAST one), the sequential cut-back on a stack (a match trimmed to nothing drops out; an empty stack with matches
//             left is where the reference raises: the job is flagged and finishes on the host)
//   chain     rv_chain for two paths between the sentinels (interval begin - 1, interval end): matches in the order of path 0; lanes over the
//             predecessors, one wave reduction per match on (score + gain - wpen * gap, then the order of the host's `active` list: score descending,
//             step at which the predecessor became active ascending, sort order ascending)
//   split     the last match in chain order whose length is not smaller than any before it; the anchor is the TRIMMED match
// rv_pick_chain's stable sort by ascending l between trim and chain only decides which of several sample sets is chained and what --maxmums keeps:
// with two samples and a cap that cannot bite the chain sees the same matches in the order of path 0 either way, so it is not made here.  First
// coordinates are distinct (MUMs, and trimming keeps pieces of disjoint matches), so the dictionary collisions rv_chain handles cannot occur.
//
// LDS: k_leaf's 50 424 B (32-bit suffix arrays; 68 856 B with 64-bit ones) + one list of 8 B per rank = 16 KB.  The second list of the sorts and
// the step numbers of the chain live in the ranks [S, E) of the OTHER copy of the sub-index' arrays and of act[], which are free until the split
// writes the children there (the live frames of a root have disjoint rank ranges).  66 808 B: two workgroups per CU (k_leaf: three); the 64-bit
// library 85 240 B: one.  160 KiB per CU.  111 / 126 VGPRs, no scratch (compiler remarks).
#include "rv_leaf_stages.h"

namespace {

constexpr u32 LINK_L = 0xFFFFu;        // predecessor: the left sentinel
constexpr u32 NOT_ACTIVE = 0xFFFFu;

struct Mt { int l, a, b; };            // a match: length, position on path 0 / 1 (relative to the job's sequences)
__device__ inline u64 mt_pack(const Mt &m) { return (u64)(u32)m.l | ((u64)(u32)m.a << 16) | ((u64)(u32)m.b << 32); }
__device__ inline Mt mt_unpack(u64 w) { Mt m; m.l = (int)(w & 0xFFFFu); m.a = (int)((w >> 16) & 0xFFFFu); m.b = (int)((w >> 32) & 0xFFFFu); return m; }

// utils.gapcost for two paths (rv_chain.hip gapcost): d0, d1 = end of the predecessor - start of the match
__device__ inline int gap2(int d0, int d1, int model) {
    if (model == 1) { const int s = d0 + d1; return (s < 0 ? -s : s) / 2; }
    const int D0 = d0 < 0 ? -d0 : d0, D1 = d1 < 0 ? -d1 : d1;
    if (model == 2) return D0 > D1 ? D0 : D1;
    return D0 > D1 ? D0 - D1 : D1 - D0;
}

// the flag word of the root's JOB (the cold path: a root that cannot be finished).  The roots of a launch are whole jobs in a small round and sub-indices of
// jobs, at any level, in a large one: the host ships the job of every root with the launch (found among the round's text begins, rv_align.hip leaf_launch).
// (Searched here instead, inlined, the begins cost a VGPR and seven spilled SGPRs; out of line, 48 B of scratch.)
__device__ inline u32 *job_flag(const RvLeafChainArgs &P) { return P.flags + P.root_job[blockIdx.x]; }

struct PickChain {
    static __device__ __forceinline__ void fail(const RvLeafArgs &, const RvLeafChainArgs &P, u32 bits) { atomicOr(job_flag(P), bits); }

    static __device__ __forceinline__ bool pick(const RvLeafArgs &, const RvLeafChainArgs &P, const LeafSub &X, u32 &L, int64_t &pa, int64_t &pb) {
        __shared__ u64 eA[LN];
        const int S = X.S, E = X.E, lane = X.lane;
        u64 *la = eA + S;                                    // list A; during the chain: score (low word) | link << 32
        u32 *lb_la = X.nl + S; sa_t *lb_b = X.ns + S;         // list B: l | a << 16, b
        uint16_t *act = X.act + S;                           // chain: the step at which a match became active
        const sa_t nsep0 = X.nsep0;
        auto getB = [&](int i) { Mt m; const u32 w = lb_la[i]; m.l = (int)(w & 0xFFFFu); m.a = (int)(w >> 16); m.b = (int)lb_b[i]; return m; };
        auto putB = [&](int i, const Mt &m) { lb_la[i] = (u32)m.l | ((u32)m.a << 16); lb_b[i] = (sa_t)m.b; };
        auto done = [&](const Mt &m) { L = (u32)m.l; pa = X.ra0 + m.a; pb = X.rb0 + m.b; return true; };

        // ---- collect: the candidates of the scan predicate, in rank order ----------------------------------------------
        int m = 0;
        for (int base = S; base < E; base += 64) {
            const int i = base + lane;
            bool ok = false; Mt c; c.l = c.a = c.b = 0;
            if (i < E && i > S) {
                const u32 l = X.cl[i]; const sa_t s1 = X.cs[i], s0 = X.cs[i - 1];
                const u32 nx = (i + 1 < E) ? X.cl[i + 1] : 0u;
                ok = l >= X.minl && ((s1 > nsep0) != (s0 > nsep0)) && X.cl[i - 1] < l && nx < l &&
                     (s1 < s0 ? left_maximal(X.cb[i], X.cb[i - 1]) : left_maximal(X.cb[i - 1], X.cb[i]));
                c.l = (int)l; c.a = (int)((int64_t)(s1 < s0 ? s1 : s0) - X.ra0); c.b = (int)((int64_t)(s1 < s0 ? s0 : s1) - X.rb0);
            }
            const u64 mask = __ballot(ok);
            if (ok) la[m + (int)lanes_below(mask)] = mt_pack(c);
            m += (int)__popcll(mask);
        }
        if (!X.both || m == 0) return false;
        WSYNC();
        if (m == 1) return done(mt_unpack(la[0]));

        // list A -> list B in the stable order of (position on path c, -l): every match counts the ones in front of it
        auto sort_AB = [&](int c, int cnt) {
            for (int base = 0; base < cnt; base += 64) {
                const int i = base + lane;
                Mt me; me.l = me.a = me.b = 0;
                if (i < cnt) me = mt_unpack(la[i]);
                const u32 key = ((u32)(c ? me.b : me.a) << 12) | (u32)(4095 - me.l);
                int r = 0;
                for (int j = 0; j < cnt; j++) {
                    const Mt o = mt_unpack(la[j]);              // (the same address for every lane: one broadcast read)
                    const u32 ko = ((u32)(c ? o.b : o.a) << 12) | (u32)(4095 - o.l);
                    r += (ko < key || (ko == key && j < i)) ? 1 : 0;
                }
                if (i < cnt) putB(r, me);
            }
            WSYNC();
        };

        // ---- pk_trim_overlap (rv_pick.h; schemes.py:160-193) -------------------------------------------------------------
        for (int c = 0; c < 2 && m > 1; c++) {
            sort_AB(c, m);
            // the containment filter, B -> A
            const Mt b0 = getB(0), b1 = getB(1);
            const int end0 = (c ? b0.b : b0.a) + b0.l, end1 = (c ? b1.b : b1.a) + b1.l;
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
                if (keep) la[w + (int)lanes_below(mask)] = mt_pack(me);
                w += (int)__popcll(mask);
            }
            m = w;
            WSYNC();
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
                WSYNC();
            }
            if (raised) { if (lane == 0) atomicOr(job_flag(P), 1u); return false; }
            m = top + 1;
        }
        if (m == 0) return false;
        if (m == 1) return done(mt_unpack(la[0]));

        // ---- rv_chain for two paths ----------------------------------------------------------------------------------------
        sort_AB(0, m);                                          // the order of path 0 (distinct coordinates)
        for (int i = lane; i < m; i += 64) act[i] = (uint16_t)NOT_ACTIVE;
        WSYNC();
        const int aL = (int)(X.f.a0 - 1 - X.ra0), bL = (int)(X.f.b0 - 1 - X.rb0);      // `left`: right in front of the intervals
        const int aR = (int)(X.f.a1 - X.ra0), bR = (int)(X.f.b1 - X.rb0);              // `right`: right behind them
        const int wscore = P.wscore, wpen = P.wpen, model = P.gcmodel;
        u32 linkR = LINK_L;
        for (int e = 0; e <= m; e++) {
            Mt me; me.l = 0; me.a = aR; me.b = bR;
            if (e < m) me = getB(e);
            const int gain = wscore * me.l;                     // n (n - 1) / 2 = 1 for two members; `right` has none
            // a lane's best predecessor: k1 = candidate score, then the predecessor's score (both descending); k2 = (step of activation + 1) << 12 |
            // sort order (ascending); the left sentinel is active from the start: k2 = 0
            u64 b1 = 0; u32 b2 = 0xFFFFFFFFu;
            if (lane == 0 && aL <= me.a && bL <= me.b) {
                const int tmpw = gain - wpen * gap2(aL - me.a, bL - me.b, model);
                b1 = ((u64)((u32)tmpw ^ 0x80000000u) << 32) | (u64)(0u ^ 0x80000000u);
                b2 = 0;
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
                        const u32 k2 = ((st + 1u) << 12) | (u32)p;
                        if (k1 > b1 || (k1 == b1 && k2 < b2)) { b1 = k1; b2 = k2; }
                    }
                }
            }
            const u64 w1 = wave_max_u64(b1);
            if (w1 == 0) { if (lane == 0) atomicOr(job_flag(P), 2u); return false; }      // (a match that does not lie behind `left`: rv_chain fails)
            const u32 w2 = 0xFFFFFFFFu - (u32)wave_max_u64((u64)(0xFFFFFFFFu - (b1 == w1 ? b2 : 0xFFFFFFFFu)));
            const u32 link = w2 < 4096u ? LINK_L : (w2 & 0xFFFu);
            const u32 score = (u32)(w1 >> 32) ^ 0x80000000u;
            if (e < m) { if (lane == 0) la[e] = (u64)score | ((u64)link << 32); }
            else linkR = link;
            WSYNC();
        }
        // back from `right`: the largest of the chain, of equal lengths the last in chain order = the first met on the way back
        int split = -1, bl = 0, guard = 0;
        for (u32 c = linkR; c != LINK_L; c = (u32)(la[c] >> 32) & 0xFFFFu) {
            if (c >= (u32)m || ++guard > m) { if (lane == 0) atomicOr(job_flag(P), 2u); return false; }      // (broken back-pointer chain)
            const int l = getB((int)c).l;
            if (l > bl) { bl = l; split = (int)c; }
        }
        if (split < 0) return false;                            // `right` links to `left`: an empty chain, nothing picked
        return done(getB(split));
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
