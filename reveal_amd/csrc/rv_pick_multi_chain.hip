// rv_pick_multi_chain.hip -- the reference's default picker for the sub-indices of a level of the multi-sample level pipeline (k_pick_multi_chain), for
// rv_many's jobs of 3 .. RV_MANY_KMAX sequences above RV_LEAF_N ranks under rv_many_set_picker(1) (RV_MANY_CHAIN_LARGE_MULTI).
//
// The multi-sample level pipeline picks on the device: k_multi_pick1 / k_multi_pick2 (rv_scan.hip) keep the longest match present in every sample of a
// sub-index.  Under the multi-sample chain route of rv_many's handle (rv_multi_chain_route, rv_align.hip) the level's scan runs UNFILTERED (k_scan_multi
// with sub_want = 0: the matches of sample subsets are listed too) and this kernel is launched in place of the two pick kernels.  It writes what
// schemes.graphmumpicker (reveal/schemes.py:197-361) picks for every sub-index: the matches in every sample -- or, where there are none, the best sample
// subset (`segment`) --, their overlaps trimmed, chained, split on the largest match of the chain: the TRIMMED match, which may be shorter than minl and
// may lie in fewer samples than the sub-index holds (the host then makes a `rest` child, as on the ordinary path).  rv_pick_chain (rv_chain.hip, with
// pk_trim_overlap of rv_pick.h and rv_chain) is the specification; stages 2 .. 5 of k_leaf_multi_chain<16> (rv_leaf_multi_chain.hip) are the same
// decisions at 11-bit positions, tools/chain_multi_proto.py restates them.  This kernel is to k_leaf_multi_chain what k_pick_chain is to k_leaf_chain:
// the pick stage alone, with wider fields, reading the scan's survivors instead of scanning.
//
// Input: the lists k_scan_multi leaves in device memory -- records RvMultiRec {l, n, ub} in per-tile blocks (tiletab[t] = first record, records, ..) in the
// reference's emission order (ascending ub, of those that close at one rank the innermost first: the order of the reference's interval stack, which
// `segment` breaks its tie by).  A sub-index of ranks [r0, r1) collects the records of the tiles r0 / 512 .. (r1 - 1) / 512 whose ub lies in its range.
// The members of a record are SA[ub - n + 1 .. ub]; the scan's member lists are not read (the scan is run with a member capacity of 0).  The sample of
// a member is the one of the sub-index' intervals (one per sample: nodes[2 W s ..]) that holds it.
//
// What the caller guarantees (rv_many.hip many_chain_large_multi_admits) is what k_leaf_multi_chain<16> asks for, with other bounds:
//   trim on, minl > 0, no seed possible, a --maxmums of at least the job's ranks, gap model 0 .. 2, at most KM = 16 samples
//   a job of at most 2^17 ranks          a sub-index' intervals are pieces of its job's sequences: lengths and positions relative to the interval begins
//                                        lie in [0, 2^17) -- 17 bits each (the kernel flags a job whose interval is longer instead of packing garbage)
//   0 <= wscore, wpen <= RV_PICK_MCHAIN_WMAX = 2^9
//                                        scores in 32 bits.  A match of n members and length l covers n * l ranks of its job and the matches of a chain
//                                        are disjoint on every path: sum (n * l) <= 2^17.  A gain is wscore * (n * l) * (n - 1) / 2 with (n - 1) / 2 <= 7.5:
//                                        the gains of a chain add up to at most wscore * 7.5 * 2^17.  A sum-of-pairs gap is sum_{i<j} | |d_i| - |d_j| | <=
//                                        (n - 1) * sum |d_i|, and the |d_i| lie inside different sequences of the job: a gap cost is at most 15 * 2^17 (one
//                                        path far away, the others at hand: the bound is reached; the star models stay below 2^17).  A score is at least
//                                        what the left sentinel offers, >= -wpen * 15 * 2^17, and at most wscore * 7.5 * 2^17; a candidate score + gain -
//                                        wpen * gap lies within [-wpen * 30 * 2^17, wscore * 7.5 * 2^17].  At RV_LEAF_MCHAIN_WMAX = 2^10 that is -3.75 * 2^30:
//                                        it does NOT fit.  The bound of this class is therefore 2^9 (1.875 * 2^30 < 2^31; the products wpen * gap and wscore * l *
//                                        n (n - 1) / 2 are smaller still) -- lowered instead of widening the scores, because the tie order packs (candidate,
//                                        predecessor's score) into one 64-bit key for ONE wave reduction per match, and the reference's defaults are 1 and 1
//   with weights >= 0 the early `break` of rv_chain never changes the choice (rv_leaf_chain.hip)
//
// Packed fields:
//   a coordinate u32: position relative to the begin of its sample's interval (17 bits) | sample << 17 (4 bits).  The text is sample-major, so this order
//                is the order of the text positions pk_trim_overlap sorts member c by (member c of two matches may lie in different samples, as in the
//                reference); an end (position + l) of sample s stays below every begin of sample s + 1, here as in the text, and an overlap > 0 can only
//                be one of two members of the same sample, where the difference is exact
//   a match      u64: l (17 bits, 0 .. 16) | shift << 17 (17 bits: how far trimming moved its members) | candidate << 34 (10 bits: its row of coordinates)
//                | n << 44 (5 bits): 49 bits
//   sort keys    u64: coordinate << 18 | (2^18 - 1 - l) (trim: position ascending, longer first), first-path position << 18 | l (chain: rv_pick_chain's list
//                is in ascending l)
//   chain entry  u64: score (32 bits, two's complement) | link << 32 (16 bits; 0xFFFF = the left sentinel)
//   tie order    k1 (ONE 64-bit key, larger wins) = (candidate score ^ 2^31) << 32 | (predecessor's score ^ 2^31); among equal k1 the smaller
//                k2 = (step of activation + 1) << 16 | sort order (the left sentinel, active from the start: 0) -- k_leaf_multi_chain's key
//   the step at which a match became active, the sample set of a candidate: 16 bits each (the same array, one after the other)
//
// Lists in LDS, PM_CAP = 512 candidates per sub-index: coordinates 512 x 16 x 4 B = 32 768 B, two lists of 8 B, the first-path positions in list order
// and sorted (4 B each) and the 16-bit array: 13 312 B; with the per-sample tables 46.6 KB per workgroup: three workgroups per CU (160 KiB).  What counts against the cap is what
// the picker chains: the matches in every sample -- all of the list only where `segment` has to choose.  A sub-index with more flags its job (bit 32)
// and gets no pick; RV_PICK_MCHAIN_CAP (test hook, in the spirit of RV_PICK_CHAIN_CAP) lowers the cap so that this is reachable at small shapes.
//
// Shape: ONE wavefront per sub-index, a workgroup of 64 threads (rv_pick_chain.hip argues the shape: the chain visits its matches one after the other,
// each with a reduction over its predecessors; several wavefronts per sub-index would put a workgroup barrier behind every match, the cut-back of the
// trim cannot be divided at all, and a level holds many sub-indices).  The wavefront holds four predecessors of a chain step, sixteen lanes (one per
// sample) each, as k_leaf_multi_chain<16>.  The rank sorts are quadratic in the candidates: 512^2 / 64 = 4096 trips at the cap, one sort per member index
// of the set and one for the chain.
//
// The flag word is the JOB's (1: trim_overlap raises in the reference, 2: broken chain or a match outside the intervals, 8: another match has the split's
// offsets member by member -- rv_pick_chain's `mapping` would hand out that one --, 32: over the cap, 64: an interval too long for the fields).  The job of
// a sub-index comes from the round's job table: begins[q * njobs + j] = where sequence q of job j begins in the text (ManyDevJobK::beg[q], and for a job
// without a q-th sequence the begin of the next one that has it, so that every row ascends); the sub-index' lowest live sample is looked up in its row
// by binary search, as job_of of rv_pick_chain.hip does.  The same row entry is the sequence begin the offsets of `mapping` are relative to.
// The template parameter is the sample bound; only the 16-sample form is instantiated (the jobs of 17 .. 64 sequences above RV_LEAF_N ranks stay ordinary
// under a picker).  No scratch, no VGPR spill (compiler remarks; DESIGN.md 3j quotes them).
#include "rv_scan.h"

namespace {

constexpr int PM_CAP = RV_PICK_MCHAIN_CAP_MAX;
constexpr u32 LINK_L = 0xFFFFu, NOT_ACTIVE = 0xFFFFu;
constexpr int POS_BITS = 17;
constexpr u32 POS_MASK = (1u << POS_BITS) - 1;
static_assert(PM_CAP <= 1024, "the candidate's row in ten bits of a match; links, sort order and activation steps in 16");

#define PM_WSYNC() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier(); } while (0)

// a match of the lists: length after trimming, how far trimming moved its members, its row of coordinates, members
struct Mt { int l, sh, ci, n; };
__device__ inline u64 mt_pack(const Mt &m) { return (u64)(u32)m.l | ((u64)(u32)m.sh << 17) | ((u64)(u32)m.ci << 34) | ((u64)(u32)m.n << 44); }
__device__ inline Mt mt_unpack(u64 w) { Mt m; m.l = (int)(w & POS_MASK); m.sh = (int)((w >> 17) & POS_MASK); m.ci = (int)((w >> 34) & 0x3FFu); m.n = (int)((w >> 44) & 0x1Fu); return m; }
__device__ inline u32 pm_lanes_below(u64 mask) { return __builtin_amdgcn_mbcnt_hi((u32)(mask >> 32), __builtin_amdgcn_mbcnt_lo((u32)mask, 0u)); }
__device__ inline int pm_iabs(int x) { return x < 0 ? -x : x; }
__device__ inline int pm_group_sum(int v) { v += __shfl_xor(v, 8, 16); v += __shfl_xor(v, 4, 16); v += __shfl_xor(v, 2, 16); v += __shfl_xor(v, 1, 16); return v; }

// the job whose sequence (of the row's sample) holds text position p: the last begin at or in front of it
__device__ inline int pm_job_of(const int64_t *__restrict__ beg, int njobs, int64_t p) {
    int lo = 0, hi = njobs;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (beg[mid] <= p) lo = mid + 1; else hi = mid; }
    return lo > 0 ? lo - 1 : 0;
}

template <int KM>
__global__ __launch_bounds__(64) void k_pick_multi_chain(const sa_t *__restrict__ SA, const RvMultiRec *__restrict__ rec, u32 rec_cap, const uint4 *__restrict__ tiletab,
                                                         int64_t ntile, const int64_t *__restrict__ sub_start, int nsubs, u32 *__restrict__ pick_l,
                                                         u32 *__restrict__ pick_n, sa_t *__restrict__ pick_pos, RvPickMultiChainArgs P) {
    static_assert(KM == 16, "four predecessors a chain step, sixteen lanes each; sample sets in 16 bits; the sample in four bits of a coordinate");
    constexpr int GRPS = 64 / KM;
    __shared__ u32 crd[PM_CAP][KM];        // the members of every candidate, in member (rank) order
    __shared__ u64 la[PM_CAP], lbk[PM_CAP];
    __shared__ u32 pun[PM_CAP], skey[PM_CAP];      // chain: the positions on the first path in list order, and sorted
    __shared__ uint16_t aux[PM_CAP];       // the candidates' sample sets, then the chain's steps of activation
    __shared__ int64_t ib[KM];             // per sample: where its interval begins in the text
    __shared__ int ilen[KM], ioff[KM];     // ... its length (0: the sub-index does not hold the sample), its begin relative to its sequence
    __shared__ u32 cme[KM], cpr[GRPS][KM]; // chain: the match's / the step's predecessors' positions per sample
    const int s = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int W = P.W;
    if (s >= nsubs || W < 2 || W > KM) return;
    const int sl = lane & (KM - 1), grp = lane / KM;
    // ---- the sub-index: its intervals, its job ----
    int64_t myb = 0, mye = 0;
    if (lane < W) { myb = (int64_t)P.nodes[(size_t)s * 2 * W + 2 * lane]; mye = (int64_t)P.nodes[(size_t)s * 2 * W + 2 * lane + 1]; }
    const bool lv = myb < mye;
    const u64 live = __ballot(lv);
    const int nsub = (int)__popcll(live);
    if (nsub < 2) return;                                     // one sample only: no match, no pick
    const int q0 = (int)__builtin_ctzll(live);
    const int64_t b_q0 = ((int64_t)(u32)__builtin_amdgcn_readlane((int)(u32)(myb >> 32), q0) << 32) | (int64_t)(u32)__builtin_amdgcn_readlane((int)(u32)myb, q0);
    const int job = pm_job_of(P.job_begin + (size_t)q0 * P.njobs, P.njobs, b_q0);
    auto flag_job = [&](u32 bits) { if (lane == 0) atomicOr(&P.job_flags[job], bits); };
    if (__ballot(lv && mye - myb >= ((int64_t)1 << POS_BITS))) { flag_job(64u); return; }
    if (lane < KM) {
        ib[lane] = myb; ilen[lane] = lv ? (int)(mye - myb) : 0;
        ioff[lane] = lv ? (int)(myb - P.job_begin[(size_t)lane * P.njobs + job]) : 0;
    }
    PM_WSYNC();
    const int64_t r0 = sub_start[s], r1 = sub_start[s + 1];
    const int cap = (int)(P.cap < (u32)PM_CAP ? P.cap : (u32)PM_CAP);

    // ---- count: the records of this sub-index, and those in every one of its samples ----
    const int64_t t0 = r0 / RV_MULTI_TILE, t1 = (r1 - 1) / RV_MULTI_TILE;
    int m_all = 0, nfull = 0;
    for (int64_t t = t0; t <= t1 && t < ntile; t++) {
        const uint4 e = tiletab[t];
        for (u32 qb = 0; qb < e.y; qb += 64) {
            const u32 q = qb + (u32)lane;
            bool ok = false, full = false;
            if (q < e.y && e.x + q < rec_cap) {
                const RvMultiRec r = rec[e.x + q];
                ok = (int64_t)r.ub >= r0 && (int64_t)r.ub < r1;
                full = ok && (int)r.n == nsub;
            }
            m_all += (int)__popcll(__ballot(ok)); nfull += (int)__popcll(__ballot(full));
        }
    }
    if (m_all == 0) return;
    const bool segment = nfull == 0;
    if (segment && nsub <= 2) return;
    int m = segment ? m_all : nfull;
    if (m > cap) { flag_job(32u); return; }

    // ---- collect, in emission order: the coordinates of the members, the sample set ----
    {
        int at0 = 0;
        bool bad = false;
        for (int64_t t = t0; t <= t1 && t < ntile; t++) {
            const uint4 e = tiletab[t];
            for (u32 qb = 0; qb < e.y; qb += 64) {
                const u32 q = qb + (u32)lane;
                bool ok = false;
                RvMultiRec r; r.l = r.n = r.ub = r.pad = 0;
                if (q < e.y && e.x + q < rec_cap) {
                    r = rec[e.x + q];
                    ok = (int64_t)r.ub >= r0 && (int64_t)r.ub < r1 && (segment || (int)r.n == nsub);
                }
                if (ok && (r.n < 2u || r.n > (u32)KM || (int64_t)r.ub - (int64_t)r.n + 1 < r0 || r.l == 0u || r.l > POS_MASK)) { ok = false; bad = true; }
                const u64 mask = __ballot(ok);
                const int at = at0 + (int)pm_lanes_below(mask);
                if (ok && at < m) {
                    u32 set = 0;
                    for (u32 c = 0; c < r.n; c++) {
                        const int64_t p = (int64_t)SA[(int64_t)r.ub - (int64_t)r.n + 1 + c];
                        int j = -1;
                        for (int x = 0; x < W; x++) if (ilen[x] > 0 && p >= ib[x] && p < ib[x] + ilen[x]) j = x;
                        if (j < 0 || p + (int64_t)r.l > ib[j] + ilen[j] || ((set >> j) & 1u)) { bad = true; j = 0; crd[at][c] = 0; }
                        else crd[at][c] = ((u32)j << POS_BITS) | (u32)(p - ib[j]);
                        set |= 1u << j;
                    }
                    Mt c; c.l = (int)r.l; c.sh = 0; c.ci = at; c.n = (int)r.n;
                    la[at] = mt_pack(c); aux[at] = (uint16_t)set;
                }
                at0 += (int)__popcll(mask);
            }
        }
        if (__ballot(bad) || at0 != m) { flag_job(2u); return; }      // (a match outside the intervals; a list that changed between the two passes)
    }
    PM_WSYNC();

    // ---- the set: every sample of the sub-index, or `segment` (schemes.py:107-126): group by sample set, z = (sum of l) x (members), strict > in first-seen order ----
    u32 setmask = (u32)live;
    if (segment) {
        u64 best = 0;
        for (int base = 0; base < m; base += 64) {
            const int i = base + lane;
            if (i < m) {
                const u32 mk = aux[i];
                u32 z = 0; int first = -1;
                for (int j = 0; j < m; j++) if ((u32)aux[j] == mk) { z += (u32)(la[j] & POS_MASK); if (first < 0) first = j; }
                z *= (u32)__builtin_popcount(mk);
                const u64 key = ((u64)z << 32) | (u64)(0xFFFFu - (u32)first);
                best = key > best ? key : best;
            }
        }
        best = rv_wave_max_u64(best);
        if (best == 0) return;
        setmask = aux[(int)(0xFFFFu - (u32)(best & 0xFFFFu))];
        int w = 0;                                            // the chosen matches, in list order, to the front of list A
        for (int base = 0; base < m; base += 64) {
            const int i = base + lane;
            const bool keep = i < m && (u32)aux[i] == setmask;
            const u64 recw = i < m ? la[i] : 0ull;
            PM_WSYNC();
            const u64 mask = __ballot(keep);
            if (keep) la[w + (int)pm_lanes_below(mask)] = recw;
            w += (int)__popcll(mask);
            PM_WSYNC();
        }
        m = w;
        if (m == 0) return;
    }
    setmask = (u32)__builtin_amdgcn_readfirstlane((int)setmask);
    const int kset = __builtin_popcount(setmask);
    auto posc = [&](const Mt &x, int c) { return (int)crd[x.ci][c] + x.sh; };
    // list A -> list B in the stable order of (position of member c, -l): every match counts the ones in front of it
    auto sort_AB = [&](int c, int cnt) {
        for (int base = 0; base < cnt; base += 64) {
            const int i = base + lane;
            u64 key = 0, me = 0;
            if (i < cnt) { me = la[i]; const Mt x = mt_unpack(me); key = ((u64)(u32)posc(x, c) << 18) | (u64)(262143u - (u32)x.l); }
            int r = 0;
            for (int j = 0; j < cnt; j++) {
                const Mt o = mt_unpack(la[j]);                // (the same address for every lane: one broadcast read)
                const u64 ko = ((u64)(u32)posc(o, c) << 18) | (u64)(262143u - (u32)o.l);
                r += (ko < key || (ko == key && j < i)) ? 1 : 0;
            }
            if (i < cnt) lbk[r] = me;
        }
        PM_WSYNC();
    };

    // ---- pk_trim_overlap (rv_pick.h; schemes.py:160-193) over every member index ----
    for (int c = 0; c < kset && m > 1; c++) {
        sort_AB(c, m);
        const Mt f0 = mt_unpack(lbk[0]), f1 = mt_unpack(lbk[1]);
        const int end0 = posc(f0, c) + f0.l, end1 = posc(f1, c) + f1.l;
        int w = 0;
        for (int base = 0; base < m; base += 64) {
            const int i = base + lane;
            bool keep = false; u64 me = 0;
            if (i < m) {
                me = lbk[i];
                const Mt x = mt_unpack(me), pv = mt_unpack(lbk[i == 0 ? m - 1 : i - 1]);      // (i - 1 == -1: the last one)
                const int en = posc(x, c) + x.l, ep = posc(pv, c) + pv.l;
                keep = (i == 0 && end1 > end0) || ep < en;
            }
            const u64 mask = __ballot(keep);
            if (keep) la[w + (int)pm_lanes_below(mask)] = me;
            w += (int)__popcll(mask);
        }
        m = w;
        PM_WSYNC();
        if (m <= 1) break;
        // the cut-back: `trimmed` is the stack la[0 .. top], written in place.  Every lane follows the same values (broadcast reads), lane 0 writes.
        int top = 0;
        bool raised = false;
        for (int i = 1; i < m; i++) {
            if (top < 0) { raised = true; break; }            // trimmed[-1] of an empty list: the reference raises IndexError
            const Mt mum = mt_unpack(la[i]);
            Mt pm = mt_unpack(la[top]);
            const int overlap = posc(pm, c) + pm.l - posc(mum, c);
            if (overlap > 0) {
                if (pm.l - overlap > 0) { pm.l -= overlap; if (lane == 0) la[top] = mt_pack(pm); }
                else top--;
                if (mum.l - overlap > 0) {
                    Mt t = mum; t.l -= overlap; t.sh += overlap;
                    top++;
                    if (lane == 0) la[top] = mt_pack(t);
                }
            } else {
                top++;
                if (lane == 0) la[top] = mt_pack(mum);
            }
            PM_WSYNC();
        }
        if (raised) { flag_job(1u); return; }
        m = top + 1;
    }
    if (m == 0) return;
    int split = 0;
    if (m == 1) { if (lane == 0) lbk[0] = la[0]; PM_WSYNC(); }
    else {
        // ---- rv_chain over the paths of the set ----
        const int s0 = __builtin_ctz(setmask);
        for (int i = lane; i < m; i += 64) {                  // the coordinate on the first path
            const Mt x = mt_unpack(la[i]);
            u32 p0 = 0;
            for (int q = 0; q < x.n; q++) { const u32 v = crd[x.ci][q]; if ((int)(v >> POS_BITS) == s0) p0 = (v & POS_MASK) + (u32)x.sh; }
            pun[i] = p0;
        }
        PM_WSYNC();
        // rv_chain's stable sort by that coordinate over rv_pick_chain's list: ascending l, equal lengths in trim's order
        for (int base = 0; base < m; base += 64) {
            const int i = base + lane;
            u64 key = 0;
            if (i < m) key = ((u64)pun[i] << 18) | (u64)(la[i] & POS_MASK);
            int r = 0;
            for (int j = 0; j < m; j++) { const u64 ko = ((u64)pun[j] << 18) | (u64)(la[j] & POS_MASK); r += (ko < key || (ko == key && j < i)) ? 1 : 0; }
            if (i < m) { lbk[r] = la[i]; skey[r] = pun[i]; }
        }
        PM_WSYNC();
        for (int i = lane; i < m; i += 64) aux[i] = (uint16_t)NOT_ACTIVE;
        PM_WSYNC();
        const bool inset = (setmask >> sl) & 1u;
        const int ge = ilen[sl];
        const int wscore = P.wscore, wpen = P.wpen, model = P.gcmodel;
        u32 linkR = LINK_L;
        for (int e = 0; e <= m; e++) {
            Mt me; me.l = 0; me.sh = 0; me.ci = 0; me.n = 0;
            if (e < m) {
                me = mt_unpack(lbk[e]);
                if (lane < me.n) { const u32 v = crd[me.ci][lane]; cme[v >> POS_BITS] = (v & POS_MASK) + (u32)me.sh; }
            }
            PM_WSYNC();
            const int mst = e < m ? (int)cme[sl] : ge;        // where the match starts on this lane's sample; `right`: the interval's end
            const int gain = wscore * me.l * ((me.n * (me.n - 1)) / 2);
            u64 b1 = 0; u32 b2 = 0xFFFFFFFFu;
            for (int base = -1; base < e; base += GRPS) {
                const int p = base + grp;                     // this group's predecessor; -1: the left sentinel
                const bool on = p < e;
                Mt o; o.l = 0; o.sh = 0; o.ci = 0; o.n = 0;
                if (on && p >= 0) {
                    o = mt_unpack(lbk[p]);
                    if (sl < o.n) { const u32 v = crd[o.ci][sl]; cpr[grp][v >> POS_BITS] = (v & POS_MASK) + (u32)o.sh; }
                }
                PM_WSYNC();
                const int pend = p < 0 ? -1 : (int)cpr[grp][sl] + o.l;
                const int d = (on && inset) ? pend - mst : 0;
                const u32 late = (u32)(__ballot(d > 0) >> (16 * grp)) & 0xFFFFu;      // lanes where the predecessor does not end in front of the match
                // utils.gapcost over the set's paths
                const int D = pm_iabs(d);
                int acc = 0, rank = 0;
                if (model != 1) {
                    for (int j = 0; j < KM; j++) {
                        const int od = __shfl(D, (lane & 48) | j);
                        if (inset && ((setmask >> j) & 1u)) {
                            if (j > sl) acc += pm_iabs(D - od);
                            rank += (od < D || (od == D && j < sl)) ? 1 : 0;
                        }
                    }
                }
                int gap;
                if (model == 1) gap = pm_iabs(pm_group_sum(d)) / kset;
                else if (model == 2) gap = pm_group_sum((inset && rank == kset / 2) ? D : 0);
                else gap = pm_group_sum(acc);
                if (on && late == 0 && sl == 0) {
                    u32 st = 0; int sc = 0;
                    if (p >= 0) {
                        st = aux[p];
                        if (st == NOT_ACTIVE) { st = (u32)e; aux[p] = (uint16_t)e; }
                        st += 1u;
                        sc = (int)(u32)(la[p] & 0xFFFFFFFFull);
                    }
                    const int tmpw = sc + gain - wpen * gap;
                    const u64 k1 = ((u64)((u32)tmpw ^ 0x80000000u) << 32) | (u64)((u32)sc ^ 0x80000000u);
                    const u32 k2 = p < 0 ? 0u : ((st << 16) | (u32)p);
                    if (k1 > b1 || (k1 == b1 && k2 < b2)) { b1 = k1; b2 = k2; }
                }
                PM_WSYNC();
            }
            const u64 w1 = rv_wave_max_u64(b1);
            if (w1 == 0) { flag_job(2u); return; }            // (a match that does not lie behind `left`: rv_chain fails)
            const u32 w2 = 0xFFFFFFFFu - (u32)rv_wave_max_u64((u64)(0xFFFFFFFFu - (b1 == w1 ? b2 : 0xFFFFFFFFu)));
            // rv_chain keeps score and link per first-path coordinate: matches that share it share the entry (they stand side by side here, and none of them
            // is a predecessor before the last of them is through), the last one's values stand, and a link leads to the last match of the predecessor's
            // coordinate
            u32 link = w2 < 65536u ? LINK_L : (w2 & 0xFFFFu);
            if (link != LINK_L) while ((int)link + 1 < m && skey[link + 1] == skey[link]) link++;
            const u32 score = (u32)(w1 >> 32) ^ 0x80000000u;
            if (e < m) { if (lane == 0) for (int j = e; j >= 0 && skey[j] == skey[e]; j--) la[j] = (u64)score | ((u64)link << 32); }
            else linkR = link;
            PM_WSYNC();
        }
        // back from `right`: the largest of the chain, of equal lengths the last in chain order = the first met on the way back
        split = -1;
        int bl = 0, guard = 0;
        for (u32 c = linkR; c != LINK_L; c = (u32)(la[c] >> 32) & 0xFFFFu) {
            if (c >= (u32)m || ++guard > m) { flag_job(2u); return; }      // (broken back-pointer chain)
            const int l = (int)(lbk[c] & POS_MASK);
            if (l > bl) { bl = l; split = (int)c; }
        }
        if (split < 0) return;                                // `right` links to `left`: an empty chain, nothing picked
    }
    const Mt Pk = mt_unpack(lbk[split]);
    // rv_pick_chain's `mapping`: keyed by the offsets (relative to the sequence begins) member by member -- another match with the split's offsets would replace it
    bool twin = false;
    for (int base = 0; base < m; base += 64) {
        const int i = base + lane;
        if (i < m && i != split) {
            const Mt x = mt_unpack(lbk[i]);
            bool same = x.n == Pk.n;
            for (int q = 0; same && q < Pk.n; q++) {
                const u32 va = crd[x.ci][q], vb = crd[Pk.ci][q];
                same = (int)(va & POS_MASK) + x.sh + ioff[va >> POS_BITS] == (int)(vb & POS_MASK) + Pk.sh + ioff[vb >> POS_BITS];
            }
            twin |= same;
        }
    }
    if (__ballot(twin)) { flag_job(8u); return; }
    // ---- the pick: the trimmed match, members in member (rank) order ----
    if (lane == 0) { pick_l[s] = (u32)Pk.l; pick_n[s] = (u32)Pk.n; }
    if (lane < Pk.n) { const u32 v = crd[Pk.ci][lane]; pick_pos[(size_t)s * W + lane] = (sa_t)(ib[v >> POS_BITS] + (int64_t)(v & POS_MASK) + (int64_t)Pk.sh); }
}

}  // namespace

int rv_pick_multi_chain_launch(Workspace &ws, const sa_t *SA, const RvMultiRec *rec, u32 rec_cap, const uint4 *tiletab, int64_t ntile, const int64_t *sub_start,
                               int nsubs, u32 *pick_l, u32 *pick_n, sa_t *pick_pos, const RvPickMultiChainArgs &c) {
    if (nsubs <= 0 || !c.nodes || !c.job_flags || !c.job_begin || c.njobs <= 0 || c.W < 2 || c.W > RV_PICK_MCHAIN_KMAX || c.wscore < 0 || c.wpen < 0 ||
        c.wscore > RV_PICK_MCHAIN_WMAX || c.wpen > RV_PICK_MCHAIN_WMAX || c.gcmodel < 0 || c.gcmodel > 2) {
        rv_set_error("rv_pick_multi_chain_launch: arguments the chain pick of the multi-sample level pipeline does not take");
        return -1;
    }
    hipLaunchKernelGGL(k_pick_multi_chain<RV_PICK_MCHAIN_KMAX>, dim3((unsigned)nsubs), dim3(64), 0, ws.stream, SA, rec, rec_cap, tiletab, ntile, sub_start, nsubs,
                       pick_l, pick_n, pick_pos, c);
    RV_LAUNCH_CHECK();
    return 0;
}
