// rv_chain_stage.h -- the ONE device copy of what the reference's default picker decides (schemes.graphmumpicker, reveal/schemes.py:160-361): trim the
// overlaps of a sub-index' matches, chain them, split on the largest match of the chain.  rv_pick_chain (rv_chain.hip, with pk_trim_overlap of rv_pick.h
// and rv_chain) is the host specification; tools/chain_multi_proto.py restates the multi-sample stage.  Four kernels run the stage, each for one wavefront
// per sub-index, and differ only in where the lists live and how wide the packed fields are:
//   k_leaf_chain (rv_leaf_chain.hip)                     rv_chain_stage_pair    lists in the dead ranks of the leaf kernel's arrays, 16-bit positions
//   k_pick_chain (rv_pick_chain.hip)                     rv_chain_stage_pair    own LDS lists, 17-bit positions
//   k_leaf_multi_chain<16 / 64> (rv_leaf_multi_chain.hip) rv_chain_stage_multi   up to 16 / 64 samples, positions below 2^11
//   k_pick_multi_chain<16 / 64> (rv_pick_multi_chain.hip) rv_chain_stage_multi  up to 16 / 64 samples, 17-bit positions
// A kernel collects its matches into list A, hands the stage a traits object (storage accessors + field widths) and acts on the outcome:
//   RV_STAGE_NONE   nothing to pick          RV_STAGE_PICK   the pick is the TRIMMED match handed back          > 0   flag bits for the job:
//   1  trim_overlap raises in the reference      2  the chain finds no predecessor / a broken back-pointer chain
//   8  (multi) another match of the list has the split's offsets member by member: rv_pick_chain's `mapping` would hand out that one
// Everything here is __forceinline__ into the kernel; the header declares no __shared__ storage.  Every lane of the wavefront follows the same control
// flow; the lists are read by broadcast and written by the lane that owns the entry (lane 0 in the sequential parts), with RV_WSYNC between the two.
//
// What a traits type T supplies (both stages):
//   T::Mt, T::key_t                 the match record (RvMt2 / RvMtK) and the integer type of a sort key
//   T::CAP, T::LMAX                 the most matches a list holds, the longest match
//   T::COORD_BITS                   bits of a position as pos() returns it       T::LKEY_BITS    bits of the length field of a sort key
//   T::ORDER_BITS                   bits of the sort order in the tie key k2
//   getA / putA, getB / putB        list A and list B as matches                 getE / putE     a chain entry (it lives where list A did)
//   getStep / putStep               the step at which a match became active (16 bits, RV_NOT_ACTIVE = not yet)
//   pos(x, c), cut(x, overlap)      the position of match x on coordinate c; x with `overlap` bases cut off its front
//   wscore, wpen, model             the weights and the gap model (0 sum of pairs, 1 star-avg, 2 star-med)
// The pair stage also reads the sentinels aL, bL (`left`: right in front of the intervals) and aR, bR (`right`: right behind them); the multi stage
// takes them per lane and needs what rv_chain_stage_multi lists.
//
// Packed fields:
//   sort key     position << LKEY_BITS | (2^LKEY_BITS - 1 - l): smaller = in front (position ascending, longer first); the chain's first-path sort of
//                the multi stage: position << LKEY_BITS | l (rv_pick_chain's list is in ascending l)
//   chain entry  u64: score (32 bits, two's complement) | link << 32 (16 bits; RV_LINK_L = the left sentinel)
//   tie order    k1 (ONE 64-bit key, larger wins) = (candidate score ^ 2^31) << 32 | (predecessor's score ^ 2^31); among equal k1 the smaller
//                k2 = (step of activation + 1) << ORDER_BITS | sort order (the left sentinel, active from the start: 0).  That is the order of the
//                host's `active` list: score descending, step at which the predecessor became active ascending, sort order ascending
// The widths are checked below (RvStageWidths): a combination that does not fit does not compile.
//
// Scores are 32 bits because k1 packs two of them for ONE wave reduction per match.  A candidate score is score + gain - wpen * gap; the kernel that
// owns a class of jobs bounds its weights (its WMAX) so that |score| + gain + wpen * gap stays below 2^31 for the longest chain and the widest gap of
// that class, and says how next to its launch wrapper's check.  With weights >= 0 the early `break` of rv_chain never changes the choice (a later
// predecessor's score + gain is already below the best found), so the stage looks at every predecessor.
#pragma once
#include "rv_common.h"

namespace {

constexpr u32 RV_LINK_L = 0xFFFFu;         // predecessor: the left sentinel
constexpr u32 RV_NOT_ACTIVE = 0xFFFFu;
constexpr int RV_STAGE_NONE = 0, RV_STAGE_PICK = -1;

template <class T>
struct RvStageWidths {
    static_assert(T::CAP <= (1 << T::ORDER_BITS), "the sort order of a match fits the low field of k2");
    static_assert(((u64)(T::CAP + 2) << T::ORDER_BITS) < 0xFFFFFFFFull, "k2 = (step + 1) << ORDER_BITS | order in 32 bits, below the 'none yet' value");
    static_assert(T::COORD_BITS + T::LKEY_BITS <= 8 * (int)sizeof(typename T::key_t), "position and length of a sort key fit the key type");
    static_assert(T::LMAX < (1 << T::LKEY_BITS), "2^LKEY_BITS - 1 - l of a sort key does not wrap");
    static_assert(T::CAP < (int)RV_LINK_L && T::CAP < (int)RV_NOT_ACTIVE, "links and steps are 16-bit fields; RV_LINK_L / RV_NOT_ACTIVE are no valid index or step");
    static constexpr bool ok = true;
};

// utils.gapcost for two paths (rv_chain.hip gapcost): d0, d1 = end of the predecessor - start of the match
__device__ inline int rv_gap2(int d0, int d1, int model) {
    if (model == 1) { const int s = d0 + d1; return (s < 0 ? -s : s) / 2; }
    const int D0 = d0 < 0 ? -d0 : d0, D1 = d1 < 0 ? -d1 : d1;
    if (model == 2) return D0 > D1 ? D0 : D1;
    return D0 > D1 ? D0 - D1 : D1 - D0;
}

// a match of two samples: length, position on path 0 / 1; packed l | a << PB | b << 2 PB
struct RvMt2 { int l, a, b; };
template <int PB> __device__ __forceinline__ u64 rv_mt2_pack(const RvMt2 &m) { return (u64)(u32)m.l | ((u64)(u32)m.a << PB) | ((u64)(u32)m.b << (2 * PB)); }
template <int PB> __device__ __forceinline__ RvMt2 rv_mt2_unpack(u64 w) {
    static_assert(3 * PB <= 64, "three fields in 64 bits");
    constexpr u64 MASK = (1ull << PB) - 1;
    RvMt2 m; m.l = (int)(w & MASK); m.a = (int)((w >> PB) & MASK); m.b = (int)((w >> (2 * PB)) & MASK); return m;
}

// a match of the multi-sample lists: length after trimming, how far trimming moved its members, its row (what the kernel finds its members by), members;
// packed l | sh << POS_BITS | row << 2 POS_BITS | n << (2 POS_BITS + ROW_BITS), the widths from the traits
struct RvMtK { int l, sh, row, n; };
template <class T> __device__ __forceinline__ u64 rv_mtk_pack(const RvMtK &m) {
    return (u64)(u32)m.l | ((u64)(u32)m.sh << T::POS_BITS) | ((u64)(u32)m.row << (2 * T::POS_BITS)) | ((u64)(u32)m.n << (2 * T::POS_BITS + T::ROW_BITS));
}
template <class T> __device__ __forceinline__ RvMtK rv_mtk_unpack(u64 w) {
    static_assert(2 * T::POS_BITS + T::ROW_BITS + T::N_BITS <= 64, "four fields in 64 bits");
    static_assert(T::LMAX < (1 << T::POS_BITS) && T::ROWS <= (1 << T::ROW_BITS) && T::KM < (1 << T::N_BITS), "length, shift, row and member count fit their fields");
    constexpr u64 PM = (1ull << T::POS_BITS) - 1;
    RvMtK m; m.l = (int)(w & PM); m.sh = (int)((w >> T::POS_BITS) & PM); m.row = (int)((w >> (2 * T::POS_BITS)) & ((1ull << T::ROW_BITS) - 1));
    m.n = (int)((w >> (2 * T::POS_BITS + T::ROW_BITS)) & ((1ull << T::N_BITS) - 1)); return m;
}

__device__ inline int rv_cen_count(u32 m) { return __builtin_popcount(m); }
__device__ inline int rv_cen_count(u64 m) { return (int)__popcll(m); }
__device__ inline int rv_cen_first(u32 m) { return __builtin_ctz(m); }
__device__ inline int rv_cen_first(u64 m) { return (int)__builtin_ctzll(m); }
// a word that is the same in every lane, into scalar registers
__device__ __forceinline__ u32 rv_uniform(u32 v) { return (u32)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ u64 rv_uniform(u64 v) { return ((u64)rv_uniform((u32)(v >> 32)) << 32) | (u64)rv_uniform((u32)v); }

template <class T>
__device__ __forceinline__ typename T::key_t rv_sort_key(int pos, u32 low) { return ((typename T::key_t)(u32)pos << T::LKEY_BITS) | (typename T::key_t)low; }

// list A -> list B in the stable order of (position on coordinate c, -l): every match counts the ones in front of it
template <class T>
__device__ __forceinline__ void rv_stage_sort(T &t, int lane, int c, int cnt) {
    typedef typename T::Mt Mt;
    constexpr u32 LTOP = (1u << T::LKEY_BITS) - 1u;
    for (int base = 0; base < cnt; base += 64) {
        const int i = base + lane;
        Mt me = Mt(); typename T::key_t key = 0;
        if (i < cnt) { me = t.getA(i); key = rv_sort_key<T>(t.pos(me, c), LTOP - (u32)me.l); }
        int r = 0;
        for (int j = 0; j < cnt; j++) {
            const Mt o = t.getA(j);                            // (the same address for every lane: one broadcast read)
            const typename T::key_t ko = rv_sort_key<T>(t.pos(o, c), LTOP - (u32)o.l);
            r += (ko < key || (ko == key && j < i)) ? 1 : 0;
        }
        if (i < cnt) t.putB(r, me);
    }
    RV_WSYNC();
}

// pk_trim_overlap (rv_pick.h; schemes.py:160-193) over the coordinates 0 .. ncoord - 1 of the m matches of list A -> the matches left (in list A), -1 where
// the reference raises.  For two samples a coordinate is a path; for more it is a MEMBER INDEX (member c of two matches may lie in different samples, as
// in the reference).
template <class T>
__device__ __forceinline__ int rv_stage_trim(T &t, int lane, int m, int ncoord) {
    typedef typename T::Mt Mt;
    for (int c = 0; c < ncoord && m > 1; c++) {
        rv_stage_sort(t, lane, c, m);
        // the containment filter, B -> A
        const Mt f0 = t.getB(0), f1 = t.getB(1);
        const int end0 = t.pos(f0, c) + f0.l, end1 = t.pos(f1, c) + f1.l;
        int w = 0;
        for (int base = 0; base < m; base += 64) {
            const int i = base + lane;
            bool keep = false; Mt me = Mt();
            if (i < m) {
                me = t.getB(i);
                const Mt pv = t.getB(i == 0 ? m - 1 : i - 1);      // (Python's index -1: the element in front of the first is the LAST one)
                const int en = t.pos(me, c) + me.l, ep = t.pos(pv, c) + pv.l;
                keep = (i == 0 && end1 > end0) || ep < en;
            }
            const u64 mask = __ballot(keep);
            if (keep) t.putA(w + (int)rv_lanes_below(mask), me);
            w += (int)__popcll(mask);
        }
        m = w;
        RV_WSYNC();
        if (m <= 1) break;
        // the cut-back: `trimmed` is the stack A[0 .. top], written in place (it never holds more than the i matches read so far).  Every lane follows
        // the same values (broadcast reads), lane 0 writes.
        int top = 0;
        for (int i = 1; i < m; i++) {
            if (top < 0) return -1;                            // trimmed[-1] of an empty list: the reference raises IndexError
            const Mt mum = t.getA(i);
            Mt pm = t.getA(top);
            const int overlap = t.pos(pm, c) + pm.l - t.pos(mum, c);
            if (overlap > 0) {
                if (pm.l - overlap > 0) { pm.l -= overlap; if (lane == 0) t.putA(top, pm); }
                else top--;
                if (mum.l - overlap > 0) {
                    Mt x = mum; T::cut(x, overlap);
                    top++;
                    if (lane == 0) t.putA(top, x);
                }
            } else {
                top++;
                if (lane == 0) t.putA(top, mum);
            }
            RV_WSYNC();
        }
        m = top + 1;
    }
    return m;
}

// a lane's best predecessor so far: a predecessor of score `sc` that offers the candidate score `cand`, at tie key k2
struct RvBest { u64 k1 = 0; u32 k2 = 0xFFFFFFFFu; };
__device__ __forceinline__ void rv_best_offer(RvBest &b, int cand, int sc, u32 k2) {
    const u64 k1 = ((u64)((u32)cand ^ 0x80000000u) << 32) | (u64)((u32)sc ^ 0x80000000u);
    if (k1 > b.k1 || (k1 == b.k1 && k2 < b.k2)) { b.k1 = k1; b.k2 = k2; }
}
// the wavefront's choice -> its score and link (the predecessor's sort order, RV_LINK_L for the left sentinel); false: no lane had a predecessor
template <class T>
__device__ __forceinline__ bool rv_best_of_wave(const RvBest &b, u32 &score, u32 &link) {
    const u64 w1 = rv_wave_max_u64(b.k1);
    if (w1 == 0) return false;
    const u32 w2 = 0xFFFFFFFFu - (u32)rv_wave_max_u64((u64)(0xFFFFFFFFu - (b.k1 == w1 ? b.k2 : 0xFFFFFFFFu)));
    link = w2 < (1u << T::ORDER_BITS) ? RV_LINK_L : (w2 & ((1u << T::ORDER_BITS) - 1u));
    score = (u32)(w1 >> 32) ^ 0x80000000u;
    return true;
}
template <class T>
__device__ __forceinline__ u32 rv_tie_key(u32 step, int order) { return ((step + 1u) << T::ORDER_BITS) | (u32)order; }
// the step at which predecessor p became active: now (step e), unless it was before
template <class T>
__device__ __forceinline__ u32 rv_activate(T &t, int p, int e) {
    u32 st = t.getStep(p);
    if (st == RV_NOT_ACTIVE) { st = (u32)e; t.putStep(p, (u32)e); }
    return st;
}

// back from `right` along the links of the chain entries: the largest match of the chain, of equal lengths the last in chain order = the first met on
// the way back -> its index in list B; -1: `right` links to `left`, an empty chain; -2: a broken back-pointer chain
template <class T>
__device__ __forceinline__ int rv_stage_walk_back(T &t, int m, u32 linkR) {
    int split = -1, bl = 0, guard = 0;
    for (u32 c = linkR; c != RV_LINK_L; c = (u32)(t.getE((int)c) >> 32) & 0xFFFFu) {
        if (c >= (u32)m || ++guard > m) return -2;
        const int l = t.getB((int)c).l;
        if (l > bl) { bl = l; split = (int)c; }
    }
    return split;
}

// ---- two samples ---------------------------------------------------------------------------------------------------------------------------------------
// List A holds m >= 1 collected matches (l, a, b) in rank order -- the order pick_one (rv_align.hip) hands records to rv_pick_chain.  pk_trim_overlap on
// path 0, then path 1; rv_chain for two paths between the sentinels: matches in the order of path 0, lanes over the predecessors, one wave reduction per
// match; the walk back from `right`.  rv_pick_chain's stable sort by ascending l between trim and chain only decides which of several sample sets is
// chained and what --maxmums keeps: with two samples and a cap that cannot bite the chain sees the same matches in the order of path 0 either way, so it
// is not made.  First coordinates are distinct (MUMs, and trimming keeps pieces of disjoint matches): the dictionary collisions rv_chain handles (the
// shared entries of the multi stage) cannot occur.
template <class T>
__device__ __forceinline__ int rv_chain_stage_pair(T &t, int lane, int m, RvMt2 &pick) {
    static_assert(RvStageWidths<T>::ok, "");
    RV_WSYNC();                                                // (the kernel's collect wrote list A)
    if (m > 1) {
        m = rv_stage_trim(t, lane, m, 2);
        if (m < 0) return 1;
        if (m == 0) return RV_STAGE_NONE;
    }
    if (m == 1) { pick = t.getA(0); return RV_STAGE_PICK; }
    rv_stage_sort(t, lane, 0, m);                              // the order of path 0 (distinct coordinates)
    for (int i = lane; i < m; i += 64) t.putStep(i, RV_NOT_ACTIVE);
    RV_WSYNC();
    const int aL = t.aL, bL = t.bL, wscore = t.wscore, wpen = t.wpen, model = t.model;
    u32 linkR = RV_LINK_L;
    for (int e = 0; e <= m; e++) {
        RvMt2 me; me.l = 0; me.a = t.aR; me.b = t.bR;
        if (e < m) me = t.getB(e);
        const int gain = wscore * me.l;                        // n (n - 1) / 2 = 1 for two members; `right` has none
        RvBest best;
        if (lane == 0 && aL <= me.a && bL <= me.b) rv_best_offer(best, gain - wpen * rv_gap2(aL - me.a, bL - me.b, model), 0, 0u);
        for (int base = 0; base < e; base += 64) {
            const int p = base + lane;
            if (p < e) {
                const RvMt2 o = t.getB(p);
                if (o.a + o.l <= me.a && o.b + o.l <= me.b) {      // ends at or in front of the match on both paths
                    const u32 st = rv_activate(t, p, e);
                    const int sc = (int)(u32)(t.getE(p) & 0xFFFFFFFFull);
                    rv_best_offer(best, sc + gain - wpen * rv_gap2(o.a + o.l - me.a, o.b + o.l - me.b, model), sc, rv_tie_key<T>(st, p));
                }
            }
        }
        u32 score, link;
        if (!rv_best_of_wave<T>(best, score, link)) return 2;      // (a match that does not lie behind `left`: rv_chain fails)
        if (e < m) { if (lane == 0) t.putE(e, (u64)score | ((u64)link << 32)); }
        else linkR = link;
        RV_WSYNC();
    }
    const int split = rv_stage_walk_back(t, m, linkR);
    if (split == -2) return 2;
    if (split < 0) return RV_STAGE_NONE;
    pick = t.getB(split);
    return RV_STAGE_PICK;
}

// ---- up to KM = 16 / 64 samples -------------------------------------------------------------------------------------------------------------------------
// List A holds m >= 1 collected matches in the order of the reference's interval stack (an interval is handed out when it closes; of those that close at
// one rank the innermost first), nfull of them in every one of the sub-index' ns live samples (`live`: a bit per sample).
//   set       the matches in every live sample; none and ns > 2: `segment` (schemes.py:107-126) -- group by sample set, z = (sum of l) x (members), strict
//             > in first-seen order.  The chosen matches move to the front of list A (where T::SUBSETS_LISTED says that the kernel lists the other sets'
//             matches even when there are full ones, or after `segment`)
//   trim      rv_stage_trim over every member index of the set
//   chain     rv_chain over the k paths of the set between the sentinels: matches by their coordinate on the lowest sample, then in rv_pick_chain's
//             order (ascending l, trim's order).  Matches that share that coordinate share rv_chain's dictionary entry: the last one's score and link
//             stand for all of them, and a link to one of them leads to the last.  64 / KM predecessors a step, KM lanes (one per sample) each:
//             ends-before by ballot, gapcost (sum of pairs of |d|, star-avg |sum d| / k, star-med sorted |d| at k / 2) by reductions inside the KM
//             lanes; gain = wscore * l * n (n - 1) / 2.  KM = 64: ONE predecessor a step, the paths of the set taken in turn from scalar registers
//   split     the walk back, then rv_pick_chain's `mapping`: keyed by the offsets member by member -- another match with the split's offsets would
//             replace it (flag 8)
// Lane sl = lane & (KM - 1) stands for sample sl: gl / ge are the sentinels on that sample (`left`: right in front of its interval, `right`: its end).
// What T supplies beyond the common part:
//   T::KM, T::cen_t, T::POS_BITS / ROW_BITS / N_BITS / ROWS (the packed match), T::SUBSETS_LISTED
//   member(x, q, s, p)              member q of match x: its sample and its position before trimming (pos() counts the shift in, member() does not)
//   seq_off(s)                      what turns a position of sample s into the offset inside its sequence (`mapping`)
//   getSet / putSet                 the sample set of a collected match          getPun / putPun, getKey / putKey   first-path positions: list order, sorted
//   cme[s], cpr[g * KM + s]         scratch rows: the match's / group g's predecessor's position per sample
// (getSet, getPun and getStep may share storage: each is dead before the next is written.)
template <int KM, class T>
__device__ __forceinline__ int rv_chain_stage_multi(T &t, int lane, int m, int nfull, int ns, u64 live, int gl, int ge, RvMtK &pick, typename T::cen_t &setmask) {
    static_assert(RvStageWidths<T>::ok && KM == T::KM && (KM == 16 || KM == 64), "groups of KM lanes, one lane per sample");
    typedef typename T::cen_t cen_t;
    constexpr int GRPS = 64 / KM;
    const int sl = lane & (KM - 1), grp = lane / KM;
    RV_WSYNC();                                                // (the kernel's collect wrote list A and the sets)
    cen_t want = 0;
    if (nfull > 0) want = (cen_t)live;
    else if (ns > 2) {
        u64 best = 0;
        for (int base = 0; base < m; base += 64) {
            const int i = base + lane;
            if (i < m) {
                const cen_t mk = t.getSet(i);
                u32 z = 0; int first = -1;
                for (int j = 0; j < m; j++) if (t.getSet(j) == mk) { z += (u32)t.getA(j).l; if (first < 0) first = j; }
                z *= (u32)rv_cen_count(mk);
                const u64 key = ((u64)z << 32) | (u64)(0xFFFFu - (u32)first);
                best = key > best ? key : best;
            }
        }
        best = rv_wave_max_u64(best);
        if (best == 0) return RV_STAGE_NONE;
        want = t.getSet((int)(0xFFFFu - (u32)(best & 0xFFFFu)));
    } else return RV_STAGE_NONE;
    want = rv_uniform(want);                                   // (the same word in every lane: in scalar registers for the loops over its bits)
    setmask = want;
    const int kset = rv_cen_count(want);
    if (T::SUBSETS_LISTED || nfull == 0) {                     // the chosen matches, in list order, to the front of list A
        int w = 0;
        for (int base = 0; base < m; base += 64) {
            const int i = base + lane;
            const bool keep = i < m && t.getSet(i) == want;
            RvMtK rec = RvMtK();
            if (i < m) rec = t.getA(i);
            RV_WSYNC();
            const u64 mask = __ballot(keep);
            if (keep) t.putA(w + (int)rv_lanes_below(mask), rec);
            w += (int)__popcll(mask);
            RV_WSYNC();
        }
        m = w;
        if (m == 0) return RV_STAGE_NONE;
    }
    m = rv_stage_trim(t, lane, m, kset);
    if (m < 0) return 1;
    if (m == 0) return RV_STAGE_NONE;
    int split = 0;
    if (m == 1) { t.putB(0, t.getA(0)); RV_WSYNC(); }
    else {
        const int s0 = rv_cen_first(want);
        for (int i = lane; i < m; i += 64) {                   // the coordinate on the first path
            const RvMtK x = t.getA(i);
            int p0 = 0;
            for (int q = 0; q < x.n; q++) { int s, p; t.member(x, q, s, p); if (s == s0) p0 = p + x.sh; }
            t.putPun(i, (u32)p0);
        }
        RV_WSYNC();
        // rv_chain's stable sort by that coordinate over rv_pick_chain's list: ascending l, equal lengths in trim's order
        for (int base = 0; base < m; base += 64) {
            const int i = base + lane;
            RvMtK me = RvMtK(); typename T::key_t key = 0;
            if (i < m) { me = t.getA(i); key = rv_sort_key<T>((int)t.getPun(i), (u32)me.l); }
            int r = 0;
            for (int j = 0; j < m; j++) { const typename T::key_t ko = rv_sort_key<T>((int)t.getPun(j), (u32)t.getA(j).l); r += (ko < key || (ko == key && j < i)) ? 1 : 0; }
            if (i < m) { t.putB(r, me); t.putKey(r, t.getPun(i)); }
        }
        RV_WSYNC();
        for (int i = lane; i < m; i += 64) t.putStep(i, RV_NOT_ACTIVE);
        RV_WSYNC();
        const bool inset = (want >> sl) & 1u;
        const int wscore = t.wscore, wpen = t.wpen, model = t.model;
        u32 linkR = RV_LINK_L;
        for (int e = 0; e <= m; e++) {
            RvMtK me = RvMtK();
            if (e < m) {
                me = t.getB(e);
                if (lane < me.n) { int s, p; t.member(me, lane, s, p); t.cme[s] = (typename T::crd_t)(p + me.sh); }
            }
            RV_WSYNC();
            const int mst = e < m ? (int)t.cme[sl] : ge;       // where the match starts on this lane's sample; `right`: the interval's end
            const int gain = wscore * me.l * ((me.n * (me.n - 1)) / 2);
            RvBest best;
            for (int base = -1; base < e; base += GRPS) {
                const int p = base + grp;                      // this group's predecessor; -1: the left sentinel
                const bool on = p < e;
                RvMtK o = RvMtK();
                if (on && p >= 0) {
                    o = t.getB(p);
                    if (sl < o.n) { int s, q; t.member(o, sl, s, q); t.cpr[grp * KM + s] = (typename T::crd_t)(q + o.sh); }
                }
                RV_WSYNC();
                const int pend = p < 0 ? gl : (int)t.cpr[grp * KM + sl] + o.l;
                const int d = (on && inset) ? pend - mst : 0;
                u32 late;                                      // lanes where the predecessor does not end in front of the match
                if constexpr (KM == 64) late = __ballot(d > 0) ? 1u : 0u; else late = (u32)(__ballot(d > 0) >> (16 * grp)) & 0xFFFFu;
                // utils.gapcost over the set's paths
                const int D = rv_iabs(d);
                int acc = 0, rank = 0;
                if (model != 1) {
                    if constexpr (KM == 64) {
                        // every path of the set in turn, its |d| read from its lane: the lane's share of the sum of pairs (the paths above it) and its
                        // rank among the set's |d| (ties by lane) -- nothing is kept per lane beyond the two sums
                        for (cen_t mm = want; mm; mm &= mm - 1) {
                            const int j = rv_cen_first(mm);
                            const int od = __builtin_amdgcn_readlane(D, j);
                            if (inset) {
                                if (j > sl) acc += rv_iabs(D - od);
                                rank += (od < D || (od == D && j < sl)) ? 1 : 0;
                            }
                        }
                    } else {
                        for (int j = 0; j < KM; j++) {
                            const int od = __shfl(D, (lane & 48) | j);
                            if (inset && ((want >> j) & 1u)) {
                                if (j > sl) acc += rv_iabs(D - od);
                                rank += (od < D || (od == D && j < sl)) ? 1 : 0;
                            }
                        }
                    }
                }
                int gap;
                if (model == 1) gap = rv_iabs(rv_group_sum<KM>(d)) / kset;
                else if (model == 2) gap = rv_group_sum<KM>((inset && rank == kset / 2) ? D : 0);
                else gap = rv_group_sum<KM>(acc);
                if (on && late == 0 && sl == 0) {
                    int sc = 0; u32 k2 = 0u;
                    if (p >= 0) { k2 = rv_tie_key<T>(rv_activate(t, p, e), p); sc = (int)(u32)(t.getE(p) & 0xFFFFFFFFull); }
                    rv_best_offer(best, sc + gain - wpen * gap, sc, k2);
                }
                RV_WSYNC();
            }
            u32 score, link;
            if (!rv_best_of_wave<T>(best, score, link)) return 2;      // (a match that does not lie behind `left`: rv_chain fails)
            // rv_chain keeps score and link per first-path coordinate: matches that share it share the entry (they stand side by side here, and none
            // of them is a predecessor before the last of them is through), the last one's values stand, and a link leads to the last match of
            // the predecessor's coordinate
            if (link != RV_LINK_L) while ((int)link + 1 < m && t.getKey((int)link + 1) == t.getKey((int)link)) link++;
            if (e < m) { if (lane == 0) for (int j = e; j >= 0 && t.getKey(j) == t.getKey(e); j--) t.putE(j, (u64)score | ((u64)link << 32)); }
            else linkR = link;
            RV_WSYNC();
        }
        split = rv_stage_walk_back(t, m, linkR);
        if (split == -2) return 2;
        if (split < 0) return RV_STAGE_NONE;
    }
    const RvMtK P = t.getB(split);
    bool twin = false;
    for (int base = 0; base < m; base += 64) {
        const int i = base + lane;
        if (i < m && i != split) {
            const RvMtK x = t.getB(i);
            bool same = x.n == P.n;
            for (int q = 0; same && q < P.n; q++) {
                int sa, pa, sb, pb; t.member(x, q, sa, pa); t.member(P, q, sb, pb);
                same = pa + x.sh + t.seq_off(sa) == pb + P.sh + t.seq_off(sb);
            }
            twin |= same;
        }
    }
    if (__ballot(twin)) return 8;
    pick = P;
    return RV_STAGE_PICK;
}

}  // namespace
