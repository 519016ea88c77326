// rv_pick_multi_chain.hip -- the reference's default picker for the sub-indices of a level of the multi-sample level pipeline (k_pick_multi_chain), for
// rv_many's jobs of 3 .. RV_MANY_KMAX sequences above RV_LEAF_N ranks under rv_many_set_picker(1) (RV_MANY_CHAIN_LARGE_MULTI) and, in its 64-sample form,
// for the jobs of 17 .. RV_MANY_WIDE_KMAX sequences of that size (RV_MANY_CHAIN_WIDE_LARGE).  "The two forms" below says where they differ.
//
// The multi-sample level pipeline picks on the device: k_multi_pick1 / k_multi_pick2 (rv_scan.hip) keep the longest match present in every sample of a
// sub-index.  Under the multi-sample chain route of rv_many's handle (rv_multi_chain_route, rv_align.hip) the level's scan runs UNFILTERED (k_scan_multi
// with sub_want = 0: the matches of sample subsets are listed too) and this kernel is launched in place of the two pick kernels.  It writes what
// schemes.graphmumpicker (reveal/schemes.py:197-361) picks for every sub-index: the matches in every sample -- or, where there are none, the best sample
// subset (`segment`) --, their overlaps trimmed, chained, split on the largest match of the chain: the TRIMMED match, which may be shorter than minl and
// may lie in fewer samples than the sub-index holds (the host then makes a `rest` child, as on the ordinary path).  The decision is
// rv_chain_stage_multi (rv_chain_stage.h), the one k_leaf_multi_chain runs; what is here: collecting the scan's survivors with their coordinates, the
// lists, the flags and writing the pick.
//
// Input: the lists k_scan_multi leaves in device memory -- records RvMultiRec {l, n, ub} in per-tile blocks (tiletab[t] = first record, records, ..) in the
// reference's emission order (ascending ub, of those that close at one rank the innermost first: the order of the reference's interval stack, which
// `segment` breaks its tie by).  A sub-index of ranks [r0, r1) collects the records of the tiles r0 / 512 .. (r1 - 1) / 512 whose ub lies in its range.
// The members of a record are SA[ub - n + 1 .. ub]; the scan's member lists are not read (the scan is run with a member capacity of 0).  The sample of
// a member is the one of the sub-index' intervals (one per sample: nodes[2 W s ..]) that holds it.
//
// What the caller guarantees (rv_many.hip many_class_admits, the RV_MANY_CHAIN_LARGE_MULTI row of many_classes) is what k_leaf_multi_chain<16> asks for, with other bounds:
//   trim on, minl > 0, no seed possible, a --maxmums of at least the job's ranks, gap model 0 .. 2, at most KM = 16 samples
//   a job of at most 2^17 ranks          a sub-index' intervals are pieces of its job's sequences: lengths and positions relative to the interval begins
//                                        lie in [0, 2^17) -- 17 bits each (the kernel flags a job whose interval is longer instead of packing garbage)
//   0 <= wscore, wpen <= RV_PICK_MCHAIN_WMAX = 2^9
//                                        scores in 32 bits (rv_chain_stage.h).  A match of n members and length l covers n * l ranks of its job and the matches of a chain
//                                        are disjoint on every path: sum (n * l) <= 2^17.  A gain is wscore * (n * l) * (n - 1) / 2 with (n - 1) / 2 <= 7.5:
//                                        the gains of a chain add up to at most wscore * 7.5 * 2^17.  A sum-of-pairs gap is sum_{i<j} | |d_i| - |d_j| | <=
//                                        (n - 1) * sum |d_i|, and the |d_i| lie inside different sequences of the job: a gap cost is at most 15 * 2^17 (one
//                                        path far away, the others at hand: the bound is reached; the star models stay below 2^17).  A score is at least
//                                        what the left sentinel offers, >= -wpen * 15 * 2^17, and at most wscore * 7.5 * 2^17; a candidate score + gain -
//                                        wpen * gap lies within [-wpen * 30 * 2^17, wscore * 7.5 * 2^17].  At RV_LEAF_MCHAIN_WMAX = 2^10 that is -3.75 * 2^30:
//                                        it does NOT fit.  The bound of this class is therefore 2^9 (1.875 * 2^30 < 2^31; the products wpen * gap and wscore * l *
//                                        n (n - 1) / 2 are smaller still) -- lowered instead of widening the scores; the reference's defaults are 1 and 1
//
// Packed fields (MultiPickStage; the header checks that they fit):
//   a coordinate u32: position relative to the begin of its sample's interval (17 bits) | sample << 17 (4 bits).  The text is sample-major, so this order
//                is the order of the text positions pk_trim_overlap sorts member c by (member c of two matches may lie in different samples, as in the
//                reference); an end (position + l) of sample s stays below every begin of sample s + 1, here as in the text, and an overlap > 0 can only
//                be one of two members of the same sample, where the difference is exact
//   a match      u64: l (17 bits, 0 .. 16) | shift << 17 (17 bits: how far trimming moved its members) | candidate << 34 (10 bits: its row of coordinates)
//                | n << 44 (5 bits): 49 bits
//   sort keys    u64: the length field has 18 bits (l < 2^17) under a coordinate of 21; the sort order in the tie key 16
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
// by binary search (rv_job_of).  The same row entry is the sequence begin the offsets of `mapping` are relative to.
//
// The two forms.  The template parameter KM is the sample bound; rv_pick_multi_chain_launch takes the form by the samples of the handle (W <= 16: the
// 16-sample form).  W is the widest job of the round, so a round of RV_MANY_CHAIN_WIDE_LARGE (every job has 17 sequences or more) runs the 64-sample
// form at every level: its sub-indices that have dropped to 16 or fewer live samples stay with it (one form per launch; the 16-sample form could not
// name their samples, which are numbered up to 63).  Everything above describes the 16-sample form; the 64-sample form (MultiPickStage<64>) differs in
//   shape        lane s is sample s, GRPS = 1: ONE predecessor a chain step, as in k_leaf_multi_chain<64> (rv_chain_stage.h has the gap costs over 64 lanes)
//   coordinate   position (17 bits) | sample << 17 (SIX bits): 23 bits under the 18 of a sort key's length field
//   a match      l (17) | shift << 17 (17) | candidate << 34 (8 bits: 256 rows) | n << 42 (7 bits: n <= 64): 49 bits
//   sample sets  64 bits (cen_t = u64): they do not fit the 16-bit array, which keeps the chain's steps only; the candidates' sets lie in list B, which
//                nothing else uses before trim (as in k_leaf_multi_chain<64>)
//   cap          RV_PICK_WCHAIN_CAP_MAX = 256 candidates: the coordinates are 256 x 64 x 4 B = 65 536 B, with the lists and tables 73.9 KB per workgroup
//                -- two workgroups per CU (160 KiB).  512 rows would be 128 KB of coordinates alone; a cap above 256 would keep them out of LDS
//   collect      the sample of a member by binary search over the begins of the live intervals (they ascend: the text is sample-major) instead of
//                the scan over all W intervals: 6 steps for each of up to 64 members a record, not 64.  A table that does not ascend finds the wrong
//                interval, the member then lies outside it, and the job is flagged (2): nothing is read or written out of bounds
//   score width  a job of at most 2^17 ranks: sum (n * l) <= 2^17 over a chain, a gain is wscore * (n * l) * (n - 1) / 2 with (n - 1) / 2 <= 31.5: the
//                gains of a chain add up to at most wscore * 31.5 * 2^17.  A sum-of-pairs gap is at most (n - 1) * sum |d_i| <= 63 * 2^17 (the star
//                models stay below 2^17).  A score is at least what the left sentinel offers, >= -wpen * 63 * 2^17, and at most wscore * 31.5 * 2^17; a
//                candidate score + gain - wpen * gap lies within [-wpen * 126 * 2^17, wscore * 31.5 * 2^17].  At 2^8 = 256 that is -1.97 * 2^31: it does
//                NOT fit.  The bound of this class is RV_PICK_WCHAIN_WMAX = 2^7 = 128 (126 * 2^17 * 2^7 = 1.97 * 2^30 < 2^31); the reference's
//                defaults are 1 and 1
// Neither form uses scratch or spills a VGPR (compiler remarks; DESIGN.md 3j quotes them).
#include "rv_scan.h"
#include "rv_chain_stage.h"

namespace {

template <int KM> struct Census { typedef u32 type; };       // a bit per sample: the samples of a candidate, of the picked set
template <> struct Census<64> { typedef u64 type; };

// the stage's storage (rv_chain_stage.h): the kernel's own LDS lists.  The row of a match is its candidate index: crd[row][q] is member q as sample << 17 |
// position relative to the begin of that sample's interval, so `left` is -1 on every path and `right` the interval's length
template <int KM_>
struct MultiPickStage {
    typedef RvMtK Mt; typedef u64 key_t; typedef typename Census<KM_>::type cen_t; typedef u32 crd_t;
    static constexpr int KM = KM_, POS_BITS = 17, SMP_BITS = KM_ == 16 ? 4 : 6, CAP = KM_ == 16 ? RV_PICK_MCHAIN_CAP_MAX : RV_PICK_WCHAIN_CAP_MAX;
    static constexpr int ROW_BITS = KM_ == 16 ? 10 : 8, N_BITS = KM_ == 16 ? 5 : 7, ROWS = CAP, LMAX = (1 << POS_BITS) - 1;
    static constexpr int COORD_BITS = POS_BITS + SMP_BITS, LKEY_BITS = 18, ORDER_BITS = 16;
    static constexpr bool SUBSETS_LISTED = false;          // (the kernel collects the full matches alone where there are any)
    static constexpr bool SETS_IN_B = KM_ > 16;            // (sample sets wider than the 16-bit array: in list B, free until trim)
    static constexpr u32 POS_MASK = (1u << POS_BITS) - 1;
    static_assert(KM == 16 || KM == 64, "groups of KM lanes, one lane per sample");
    static_assert(KM <= (1 << SMP_BITS) && COORD_BITS <= 32, "the sample above the position of a coordinate, in a 32-bit word");
    static_assert(KM <= 8 * (int)sizeof(cen_t) && (SETS_IN_B ? sizeof(cen_t) <= sizeof(u64) : KM <= 16), "a sample set in cen_t; in the 16-bit array or an entry of list B");
    static_assert(ROWS <= (1 << ROW_BITS) && KM < (1 << N_BITS) && 2 * POS_BITS + ROW_BITS + N_BITS <= 64, "a packed match in 64 bits");
    static_assert((size_t)CAP * KM * sizeof(u32) <= 64 * 1024, "the coordinate table stays within 64 KB of LDS");
    const u32 (*crd)[KM]; u64 *la, *lb; u32 *pun, *skey; uint16_t *aux; const int *ioff; u32 *cme, *cpr;
    int wscore, wpen, model;
    __device__ __forceinline__ Mt getA(int i) const { return rv_mtk_unpack<MultiPickStage>(la[i]); }
    __device__ __forceinline__ void putA(int i, const Mt &m) { la[i] = rv_mtk_pack<MultiPickStage>(m); }
    __device__ __forceinline__ Mt getB(int i) const { return rv_mtk_unpack<MultiPickStage>(lb[i]); }
    __device__ __forceinline__ void putB(int i, const Mt &m) { lb[i] = rv_mtk_pack<MultiPickStage>(m); }
    __device__ __forceinline__ u64 getE(int i) const { return la[i]; }
    __device__ __forceinline__ void putE(int i, u64 w) { la[i] = w; }
    __device__ __forceinline__ u32 getStep(int i) const { return aux[i]; }
    __device__ __forceinline__ void putStep(int i, u32 v) { aux[i] = (uint16_t)v; }
    __device__ __forceinline__ cen_t getSet(int i) const { if constexpr (SETS_IN_B) return (cen_t)lb[i]; else return (cen_t)aux[i]; }
    __device__ __forceinline__ void putSet(int i, cen_t v) { if constexpr (SETS_IN_B) lb[i] = (u64)v; else aux[i] = (uint16_t)v; }
    __device__ __forceinline__ u32 getPun(int i) const { return pun[i]; }
    __device__ __forceinline__ void putPun(int i, u32 v) { pun[i] = v; }
    __device__ __forceinline__ u32 getKey(int i) const { return skey[i]; }
    __device__ __forceinline__ void putKey(int i, u32 v) { skey[i] = v; }
    __device__ __forceinline__ int pos(const Mt &m, int c) const { return (int)crd[m.row][c] + m.sh; }
    static __device__ __forceinline__ void cut(Mt &m, int overlap) { m.l -= overlap; m.sh += overlap; }
    __device__ __forceinline__ void member(const Mt &m, int q, int &s, int &p) const { const u32 v = crd[m.row][q]; s = (int)(v >> POS_BITS); p = (int)(v & POS_MASK); }
    __device__ __forceinline__ int seq_off(int s) const { return ioff[s]; }
};

template <int KM>
__global__ __launch_bounds__(64) void k_pick_multi_chain(const sa_t *__restrict__ SA, const RvMultiRec *__restrict__ rec, u32 rec_cap, const uint4 *__restrict__ tiletab,
                                                         int64_t ntile, const int64_t *__restrict__ sub_start, int nsubs, u32 *__restrict__ pick_l,
                                                         u32 *__restrict__ pick_n, sa_t *__restrict__ pick_pos, RvPickMultiChainArgs P) {
    static_assert(KM == 16 || KM == 64, "four predecessors a chain step, sixteen lanes each, or one of 64 lanes (MultiPickStage checks the widths)");
    typedef MultiPickStage<KM> Stage;
    typedef typename Stage::cen_t cen_t;
    constexpr int GRPS = 64 / KM, POS_BITS = Stage::POS_BITS, PM_CAP = Stage::CAP;
    constexpr u32 POS_MASK = Stage::POS_MASK;
    __shared__ u32 crd[PM_CAP][KM];        // the members of every candidate, in member (rank) order
    __shared__ u64 la[PM_CAP], lbk[PM_CAP];
    __shared__ u32 pun[PM_CAP], skey[PM_CAP];      // chain: the positions on the first path in list order, and sorted
    __shared__ uint16_t aux[PM_CAP];       // the candidates' sample sets (KM = 16; KM = 64: in list B), then the chain's steps of activation
    __shared__ int64_t ib[KM];             // per sample: where its interval begins in the text
    __shared__ int ilen[KM], ioff[KM];     // ... its length (0: the sub-index does not hold the sample), its begin relative to its sequence
    __shared__ u32 cme[KM], cpr[GRPS][KM]; // chain: the match's / the step's predecessors' positions per sample
    __shared__ int64_t lbeg[KM == 64 ? KM : 1];      // KM = 64: the begins of the live intervals, ascending, and their samples
    __shared__ uint8_t lsmp[KM == 64 ? KM : 1];
    const int s = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int W = P.W;
    if (s >= nsubs || W < 2 || W > KM) return;
    const int sl = lane & (KM - 1);
    Stage st;
    st.crd = crd; st.la = la; st.lb = lbk; st.pun = pun; st.skey = skey; st.aux = aux; st.ioff = ioff; st.cme = cme; st.cpr = &cpr[0][0];
    // ---- the sub-index: its intervals, its job ----
    int64_t myb = 0, mye = 0;
    if (lane < W) { myb = (int64_t)P.nodes[(size_t)s * 2 * W + 2 * lane]; mye = (int64_t)P.nodes[(size_t)s * 2 * W + 2 * lane + 1]; }
    const bool lv = myb < mye;
    const u64 live = __ballot(lv);
    const int nsub = (int)__popcll(live);
    if (nsub < 2) return;                                     // one sample only: no match, no pick
    const int q0 = (int)__builtin_ctzll(live);
    const int64_t b_q0 = ((int64_t)(u32)__builtin_amdgcn_readlane((int)(u32)(myb >> 32), q0) << 32) | (int64_t)(u32)__builtin_amdgcn_readlane((int)(u32)myb, q0);
    const int job = rv_job_of(P.job_begin + (size_t)q0 * P.njobs, P.njobs, b_q0);
    auto flag_job = [&](u32 bits) { if (lane == 0) atomicOr(&P.job_flags[job], bits); };
    if (__ballot(lv && mye - myb >= ((int64_t)1 << POS_BITS))) { flag_job(64u); return; }
    if (lane < KM) {
        ib[lane] = myb; ilen[lane] = lv ? (int)(mye - myb) : 0;
        ioff[lane] = lv ? (int)(myb - P.job_begin[(size_t)lane * P.njobs + job]) : 0;
    }
    if constexpr (KM == 64) {
        if (lv) { const int at = (int)rv_lanes_below(live); lbeg[at] = myb; lsmp[at] = (uint8_t)lane; }
    }
    RV_WSYNC();
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
                const int at = at0 + (int)rv_lanes_below(mask);
                if (ok && at < m) {
                    cen_t set = 0;
                    for (u32 c = 0; c < r.n; c++) {
                        const int64_t p = (int64_t)SA[(int64_t)r.ub - (int64_t)r.n + 1 + c];
                        int j = -1;
                        if constexpr (KM == 64) {
                            int lo = 0, hi = nsub;                 // the last live interval that begins at or in front of p
                            while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (lbeg[mid] <= p) lo = mid; else hi = mid; }
                            const int x = (int)lsmp[lo];
                            if (p >= ib[x] && p < ib[x] + ilen[x]) j = x;
                        } else {
                            for (int x = 0; x < W; x++) if (ilen[x] > 0 && p >= ib[x] && p < ib[x] + ilen[x]) j = x;
                        }
                        if (j < 0 || p + (int64_t)r.l > ib[j] + ilen[j] || ((set >> j) & 1u)) { bad = true; j = 0; crd[at][c] = 0; }
                        else crd[at][c] = ((u32)j << POS_BITS) | (u32)(p - ib[j]);
                        set |= (cen_t)1 << j;
                    }
                    RvMtK c; c.l = (int)r.l; c.sh = 0; c.row = at; c.n = (int)r.n;
                    st.putA(at, c); st.putSet(at, set);
                }
                at0 += (int)__popcll(mask);
            }
        }
        if (__ballot(bad) || at0 != m) { flag_job(2u); return; }      // (a match outside the intervals; a list that changed between the two passes)
    }

    // ---- the set, trim, chain, split (rv_chain_stage.h) ----
    st.wscore = P.wscore; st.wpen = P.wpen; st.model = P.gcmodel;
    RvMtK Pk; cen_t setmask = 0;
    const int res = rv_chain_stage_multi<KM>(st, lane, m, nfull, nsub, live, -1, ilen[sl], Pk, setmask);
    if (res > 0) { flag_job((u32)res); return; }
    if (res != RV_STAGE_PICK) return;
    // ---- the pick: the trimmed match, members in member (rank) order ----
    if (lane == 0) { pick_l[s] = (u32)Pk.l; pick_n[s] = (u32)Pk.n; }
    if (lane < Pk.n) { const u32 v = crd[Pk.row][lane]; pick_pos[(size_t)s * W + lane] = (sa_t)(ib[v >> POS_BITS] + (int64_t)(v & POS_MASK) + (int64_t)Pk.sh); }
}

}  // namespace

int rv_pick_multi_chain_launch(Workspace &ws, const sa_t *SA, const RvMultiRec *rec, u32 rec_cap, const uint4 *tiletab, int64_t ntile, const int64_t *sub_start,
                               int nsubs, u32 *pick_l, u32 *pick_n, sa_t *pick_pos, const RvPickMultiChainArgs &c) {
    // the form by the samples of the handle: up to 16 the 16-sample form, above the 64-sample one, each with the weight bound its scores were derived for
    const bool wide = c.W > RV_PICK_MCHAIN_KMAX;
    const int wmax = wide ? RV_PICK_WCHAIN_WMAX : RV_PICK_MCHAIN_WMAX;
    if (nsubs <= 0 || !c.nodes || !c.job_flags || !c.job_begin || c.njobs <= 0 || c.W < 2 || c.W > RV_PICK_WCHAIN_KMAX || c.wscore < 0 || c.wpen < 0 ||
        c.wscore > wmax || c.wpen > wmax || c.gcmodel < 0 || c.gcmodel > 2) {
        rv_set_error("rv_pick_multi_chain_launch: arguments the chain pick of the multi-sample level pipeline does not take");
        return -1;
    }
    if (wide) hipLaunchKernelGGL(k_pick_multi_chain<RV_PICK_WCHAIN_KMAX>, dim3((unsigned)nsubs), dim3(64), 0, ws.stream, SA, rec, rec_cap, tiletab, ntile, sub_start, nsubs,
                                 pick_l, pick_n, pick_pos, c);
    else hipLaunchKernelGGL(k_pick_multi_chain<RV_PICK_MCHAIN_KMAX>, dim3((unsigned)nsubs), dim3(64), 0, ws.stream, SA, rec, rec_cap, tiletab, ntile, sub_start, nsubs,
                       pick_l, pick_n, pick_pos, c);
    RV_LAUNCH_CHECK();
    return 0;
}
