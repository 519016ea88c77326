// rv_leaf_multi_chain.hip -- the whole recursion of a job of 3 .. RV_MANY_KMAX samples inside one workgroup with the reference's default picker as the
// pick stage (k_leaf_multi_chain), for rv_many's RV_MANY_CHAIN_MULTI rounds under picker kind 1; and, in its wide form, of a job of up to
// RV_MANY_WIDE_KMAX = 64 samples (RV_MANY_CHAIN_WIDE: the jobs of 17 .. 64 sequences).  The kernel is a template over the sample bound KM, as k_leaf_multi
// is; "The two forms" below says where they differ.
//
// The frame of the kernel is k_leaf_multi's (rv_leaf_multi.hip: one workgroup per job, the arrays in LDS in two copies, one wavefront per sub-index,
// lane s owning sample s, a shared stack of frames); k_leaf_multi itself is untouched.  What differs is everything the picker decides.  The
// specification is the ordinary path under rv_set_picker(h, 1, ..): pick_one and the linear interval model of rv_align.hip, rv_pick_chain / rv_chain /
// gapcost of rv_chain.hip, pk_trim_overlap of rv_pick.h, the scan predicate of oracle/reveal_oracle.c ro_getmultimums (reveal.c:436-580, 227-259;
// schemes.py:20-126, 160-361).
//
// Per sub-index of `len` ranks and ns live samples:
//   scan      every multi-MUM: an LCP interval of n ranks, max(minn, 2) <= n <= ns, every member from another sample, left-maximal, both flanking LCP
//             values below l, l >= minl.  A lane owns an upper rank u and walks the windows [u - n + 1, u] for n = 2 .. ns: their l only shrinks, so
//             the valid ones come out by descending l.  Lanes by ascending u: the list is in the order of the reference's interval stack (an interval
//             is handed out when it closes; of those that close at one rank the innermost first) -- the order `segment` breaks its tie by.  An
//             LCP-interval tree over len ranks has fewer than len inner nodes: the lists are indexed from the sub-index' first rank and cannot
//             overflow.  A record is (l, first rank, shift, n): member q is cs[first + q] + shift, the members are never copied (PkItem).
//   pick      set, trim, chain and the choice of the split are rv_chain_stage_multi<KM> (rv_chain_stage.h), between the sentinels (interval begin - 1,
//             interval end) of every sample; MultiLeafStage says where its lists live
//   split     on the largest match of the chain, of equal lengths the last; the anchor is the TRIMMED match, members in member (rank) order, as the
//             ordinary path emits them.  Three children: lead and trail over the set's samples, rest = the other live samples with their whole
//             intervals; running-minimum LCP per child; bubble_sort on the leading child.  A child is visited when at least max(2, minn) of its
//             samples are at least minl long (a match of a sample SUBSET needs no more; k_leaf_multi's "every interval" rule would be wrong here)
// What the kernel leaves to the host (flag the job; its anchors are dropped and it reruns the ordinary way):
//   1   trim_overlap raises in the reference                     2   the chain finds no predecessor / a broken back-pointer chain
//   8   another match of the list has the split's offsets member by member: rv_pick_chain's `mapping` would hand out that one
//   16  rv_many's test hook                                     32  the frame stack is full
// What the caller guarantees (rv_many.hip many_class_admits, the RV_MANY_CHAIN_MULTI and RV_MANY_CHAIN_WIDE rows of many_classes): trim on, minl > 0, no seed possible, a --maxmums of at least the job's ranks (a
// sub-index has fewer candidates than ranks), gap model 0 .. 2, and
//   0 <= wscore, wpen <= RV_LEAF_MCHAIN_WMAX = 2^10: scores in 32 bits (rv_chain_stage.h).  A job has at most 2^11 ranks.  The lengths of a chain are disjoint on every
//   path: they add up to at most 2^11, and n (n - 1) / 2 <= 120 < 2^7, so the gains of a chain add up to at most wscore * 2^18.  A gap cost is at most
//   120 * 2^11 < 2^18 (sum of pairs; the star models: 2^11).  A score is at least what the left sentinel offers, >= -wpen * 2^18, and at most
//   wscore * 2^18; a candidate score + gain - wpen * gap lies within 3 * 2^10 * 2^18 < 2^30.  k_leaf_chain's bound of 2^16 would need 2^36: the bound
//   is tightened instead of widening the scores; the reference's defaults are 1 and 1.
//   KM = 64: the same constant holds.  A match of n members and length l covers n * l ranks of the job, and the matches of a chain are disjoint on every
//   path, so sum (n * l) <= 2^11; a gain is wscore * (n * l) * (n - 1) / 2 with (n - 1) / 2 < 2^5: the gains of a chain add up to less than wscore * 2^16.
//   A sum-of-pairs gap is sum_{i<j} | |d_i| - |d_j| | <= (n - 1) * sum |d_i|, the |d_i| lie inside different sequences and add up to less than 2^11:
//   a gap cost is below 63 * 2^11 < 2^17 (the star models: 2^11).  A score is >= -wpen * 2^17 (the left sentinel's offer) and < wscore * 2^16; a candidate
//   score + gain - wpen * gap lies within 2^10 * (2^17 + 2^16 + 2^17) < 3 * 2^27 < 2^30.  RV_LEAF_MCHAIN_WMAX = 2^10 serves both forms (the same
//   counting gives the 16-sample form 2^14 gains and 2^15 gaps: the bound above is not tight, and is kept).
// Frame stack: a wave goes on with the smallest visited child and leaves the others to the stack -- two frames where the size falls to a third, one
// where it halves: at most 2 log3(2048) < 14 frames wait per descent, four waves descend at once, and a frame taken from the stack starts a descent
// no longer than its parent's: MAXSTACK = 96 as in k_leaf_multi.  A full stack flags the job (32), it does not fail the call.
// The two forms (compiler remarks, gfx950):
//   KM = 16   the kernel as it was before the template: four predecessors a chain step, sixteen lanes each (four exchanges for a sum, sixteen for the ranks
//             of the |d|); sample sets in 16 bits beside the candidates (aux).  k_leaf_multi<16>'s arrays + two lists of 8 B per rank + the chain's
//             coordinate scratch: 73 104 B of LDS, two workgroups per CU; 122 VGPRs, no scratch, 116 SGPRs spilled
//   KM = 64   lane s owns path s through the whole chain step: ONE predecessor a step.  Ends-before is one 64-bit ballot; a sum is the wavefront's scan.
//             Sum of pairs and star-med need every lane's |d| against every other path's: the paths of the set are taken in turn (a loop over the bits
//             of the set, which sits in scalar registers), path j's |d| is read from lane j (v_readlane), and the lane adds | |d| - |d_j| | for j above
//             it and counts the |d_j| below its own (ties by lane): its share of the 2016 pairs and its rank among 64, in two registers -- no per-lane
//             array.  The tie key is unchanged, so the order in which predecessors are looked at does not show.  Sample sets are 64 bits: the
//             candidates' sets lie in list B, which nothing else uses before trim.  Scan windows of 2 .. 64 ranks, trim over up to 64 member indices,
//             FrameMT<64> of 264 B.  k_leaf_multi<64>'s 59 248 B + the two lists (32 768 B) + coordinate scratch: 93 168 B of LDS -- ONE workgroup
//             per CU (of gfx950's 160 KiB); 121 VGPRs, no scratch, 34 SGPRs spilled.  Two per CU would need the lists inside the dead ranks of the
//             other copy of the arrays, as k_leaf_chain keeps them: not done
#include "rv_leaf_multi.h"
#include "rv_chain_stage.h"

namespace {

constexpr int NT = 256;
constexpr int LN = RV_LEAF_N;
constexpr int NW = NT / 64;
constexpr int MAXSTACK = 96;
constexpr int ACAP = 256;
constexpr u32 INF = 0xFFFFFFFFu;
constexpr uint8_t SMP_SEP = 0x40, SMP_DONE = 0x80;      // (the sample id lies below them: KM - 1, at most six bits)

template <int KM>
struct FrameMT { uint16_t start, len, depth, buf; uint16_t b[KM], e[KM]; };      // interval [b, e) of every sample, job-local; empty: b >= e
template <int KM> struct Census { typedef u32 type; };      // a bit per sample: the samples of a match, of the picked set
template <> struct Census<RV_MANY_WIDE_KMAX> { typedef u64 type; };

__device__ inline bool is_lower_c(uint8_t c) { return c >= 'a' && c <= 'z'; }
__device__ inline u32 from_lane_below(u32 x, u32 first) { return (u32)__builtin_amdgcn_update_dpp((int)first, (int)x, 0x138 /* wave_shr:1 */, 0xf, 0xf, false); }

// the stage's storage (rv_chain_stage.h), all from the sub-index' first rank: the two lists in eA / eB; the 16-bit words of act[] hold the sample sets
// of the candidates (KM = 64: 64 bits, in list B, which nothing else uses before trim), then the first-path positions, then the steps; the sorted
// first-path positions lie in the other copy of the suffix array, which is free until the split.  The row of a match is the first rank of its interval:
// member q is cs[row + q] (job-local position; the members are never copied), its sample the smp byte of that position
template <int KM_>
struct MultiLeafStage {
    typedef RvMtK Mt; typedef u32 key_t; typedef typename Census<KM_>::type cen_t; typedef uint16_t crd_t;
    static constexpr int KM = KM_, POS_BITS = 16, ROW_BITS = 16, N_BITS = 8, ROWS = LN, CAP = LN, LMAX = LN;
    static constexpr int COORD_BITS = 12, LKEY_BITS = 12, ORDER_BITS = 12;
    static constexpr bool SUBSETS_LISTED = true;           // (the scan lists every window, whatever its sample set)
    static_assert(LN <= (1 << (COORD_BITS - 1)), "a job-local position, shifted by less than a match's length, in COORD_BITS");
    const uint16_t *cs; const uint8_t *smp; const uint16_t *seqb; u64 *la, *lb; uint16_t *aux, *skey, *cme, *cpr;
    int wscore, wpen, model;
    __device__ __forceinline__ Mt getA(int i) const { return rv_mtk_unpack<MultiLeafStage>(la[i]); }
    __device__ __forceinline__ void putA(int i, const Mt &m) { la[i] = rv_mtk_pack<MultiLeafStage>(m); }
    __device__ __forceinline__ Mt getB(int i) const { return rv_mtk_unpack<MultiLeafStage>(lb[i]); }
    __device__ __forceinline__ void putB(int i, const Mt &m) { lb[i] = rv_mtk_pack<MultiLeafStage>(m); }
    __device__ __forceinline__ u64 getE(int i) const { return la[i]; }
    __device__ __forceinline__ void putE(int i, u64 w) { la[i] = w; }
    __device__ __forceinline__ u32 getStep(int i) const { return aux[i]; }
    __device__ __forceinline__ void putStep(int i, u32 v) { aux[i] = (uint16_t)v; }
    __device__ __forceinline__ cen_t getSet(int i) const { if constexpr (KM == 64) return lb[i]; else return (cen_t)aux[i]; }
    __device__ __forceinline__ void putSet(int i, cen_t v) { if constexpr (KM == 64) lb[i] = v; else aux[i] = (uint16_t)v; }
    __device__ __forceinline__ u32 getPun(int i) const { return aux[i]; }
    __device__ __forceinline__ void putPun(int i, u32 v) { aux[i] = (uint16_t)v; }
    __device__ __forceinline__ u32 getKey(int i) const { return skey[i]; }
    __device__ __forceinline__ void putKey(int i, u32 v) { skey[i] = (uint16_t)v; }
    __device__ __forceinline__ int pos(const Mt &m, int c) const { return (int)cs[m.row + c] + m.sh; }
    static __device__ __forceinline__ void cut(Mt &m, int overlap) { m.l -= overlap; m.sh += overlap; }
    __device__ __forceinline__ void member(const Mt &m, int q, int &s, int &p) const { p = (int)cs[m.row + q]; s = (int)(smp[p] & (uint8_t)(KM - 1)); }
    __device__ __forceinline__ int seq_off(int s) const { return -(int)seqb[s]; }
};

// running minimum of the LCP values since the last rank of the leading / trailing / rest child (rv_leaf_multi.hip MinSt2, one class more)
struct MinSt3 { u32 has, v0, v1, v2; };
__device__ inline MinSt3 ms3_combine(MinSt3 a, MinSt3 b) {      // a, then b
    MinSt3 r; r.has = a.has | b.has;
    r.v0 = (b.has & 1u) ? b.v0 : (a.v0 < b.v0 ? a.v0 : b.v0);
    r.v1 = (b.has & 2u) ? b.v1 : (a.v1 < b.v1 ? a.v1 : b.v1);
    r.v2 = (b.has & 4u) ? b.v2 : (a.v2 < b.v2 ? a.v2 : b.v2);
    return r;
}
__device__ inline MinSt3 wave_incl_ms3(MinSt3 m) {
    const int lane = threadIdx.x & 63;
#define LM_STEP_(CTRL, RM, TAKE) {                                                                                    \
        MinSt3 t; t.has = rv_dpp_u32<CTRL, RM>(m.has); t.v0 = rv_dpp_u32<CTRL, RM>(m.v0); t.v1 = rv_dpp_u32<CTRL, RM>(m.v1); t.v2 = rv_dpp_u32<CTRL, RM>(m.v2);    \
        const MinSt3 c = ms3_combine(t, m);                                                                           \
        if (TAKE) m = c;                                                                                              \
    }
    RV_WAVE_SCAN_STEPS(LM_STEP_)
#undef LM_STEP_
    return m;
}

// KM: the sample bound of the form, RV_MANY_KMAX (16) or RV_MANY_WIDE_KMAX (64); a wavefront holds GRPS = 64 / KM predecessors of a chain step
template <int KM>
__global__ __launch_bounds__(NT) void k_leaf_multi_chain(RvLeafMultiArgs A, RvLeafMultiChainArgs C) {
    static_assert(KM == RV_MANY_KMAX || KM == RV_MANY_WIDE_KMAX, "the sample in KM - 1 <= 0x3F of the smp byte, lane s owns sample s, groups of KM lanes in the chain");
    constexpr uint8_t SMP_ID = (uint8_t)(KM - 1);
    constexpr int GRPS = 64 / KM;
    typedef typename Census<KM>::type cen_t;
    typedef FrameMT<KM> FrameM;
    __shared__ uint16_t sa2[2][LN], lc2[2][LN];
    __shared__ uint8_t bw2[2][LN];
    __shared__ uint8_t smp[LN];
    __shared__ uint16_t act[LN];
    __shared__ u64 eA[LN], eB[LN];                // the picker's two lists, indexed from the sub-index' first rank
    __shared__ FrameM stack[MAXSTACK];
    __shared__ FrameM cur[NW];
    __shared__ uint16_t wm[NW][KM];               // the picked match: its member on every sample of its set
    __shared__ uint16_t cme[NW][KM], cpr[NW][GRPS][KM];      // chain: the match's / the step's predecessors' coordinates per sample
    __shared__ uint16_t seqb[KM];                 // where every sequence of the job begins
    __shared__ uint16_t an_l[ACAP], an_n[ACAP], an_mo[ACAP], an_pp[LN];
    __shared__ int s_top, s_pending, s_lock, s_bad;
    __shared__ u32 s_cnt, s_nm_staged, s_part[NW];
    __shared__ unsigned long long s_base;
    __shared__ unsigned long long s_stats[4];

    const RvLeafMultiJob job = A.jobs[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n = job.n;
    if (n < 2 || n > LN) { if (tid == 0) atomicOr(A.err, 16u); return; }
    for (int i = tid; i < n; i += NT) {
        sa2[0][i] = (uint16_t)((int64_t)A.SA[job.beg + i] - job.beg); lc2[0][i] = (uint16_t)A.LCP[job.beg + i]; bw2[0][i] = A.BWT[job.beg + i] & RV_BWT_CHAR;
    }
    u32 seps = 0;
#pragma unroll
    for (int r = 0; r < 8; r++) { const int p = tid * 8 + r; if (p < n && A.T[job.beg + p] == (uint8_t)'$') seps |= 1u << r; }
    const u32 mine = (u32)__builtin_popcount(seps), incl = rv_wave_incl_sum_u32(mine);
    if (lane == 63) s_part[wv] = incl;
    if (tid < KM) { cur[0].b[tid] = 0; cur[0].e[tid] = 0; }
    if (tid == 0) {
        cur[0].start = 0; cur[0].len = (uint16_t)n; cur[0].depth = 0; cur[0].buf = 0;
        s_top = 0; s_pending = 1; s_lock = 0; s_bad = 0; s_cnt = 0; s_nm_staged = 0;
        s_stats[0] = s_stats[1] = s_stats[2] = s_stats[3] = 0;
    }
    __syncthreads();
    {
        u32 before = incl - mine, total = 0;
        for (int w = 0; w < NW; w++) { const u32 o = s_part[w]; total += o; if (w < wv) before += o; }
        bool bad = total < 2 || total > (u32)KM;
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const int p = tid * 8 + r;
            if (p >= n) break;
            if (seps >> r & 1u) {
                smp[p] = (uint8_t)(SMP_SEP | (before & SMP_ID));
                if (before < (u32)KM) cur[0].e[before] = (uint16_t)p;
                if (before + 1 < (u32)KM && p + 1 < n) cur[0].b[before + 1] = (uint16_t)(p + 1);
                before++;
            } else {
                smp[p] = (uint8_t)(before & SMP_ID);
                if (p == n - 1) bad = true;
            }
        }
        if (bad) { s_bad = 1; }
    }
    __syncthreads();
    if (tid < KM) seqb[tid] = cur[0].b[tid];
    __syncthreads();                                   // the last workgroup barrier in front of the recursion
    if (s_bad) { if (tid == 0) atomicOr(A.err, 16u); return; }

    const u32 need = A.minl > 1 ? (u32)A.minl : 1u;
    const int minn = A.minn, nmin = minn > 2 ? minn : 2;
    const u32 acap = A.stage_cap < (u32)ACAP ? A.stage_cap : (u32)ACAP;
    u32 *const jflag = C.flags + blockIdx.x;
    const int sl = lane & (KM - 1);
    u32 my_steps = 0, my_splits = 0, my_maxdepth = 0; u64 my_bp = 0;
    bool have = wv == 0;

    for (;;) {
        if (!have) {
            int got = 0;
            if (lane == 0) {
                for (;;) {
                    if (__hip_atomic_load(&s_pending, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 0) { got = -1; break; }
                    if (__hip_atomic_load(&s_top, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) > 0) {
                        while (atomicCAS(&s_lock, 0, 1) != 0) __builtin_amdgcn_s_sleep(1);
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                        const int t = s_top;
                        if (t > 0) { cur[wv] = stack[t - 1]; s_top = t - 1; got = 1; }
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                        atomicExch(&s_lock, 0);
                        if (got) break;
                    }
                    __builtin_amdgcn_s_sleep(4);
                }
            }
            got = __builtin_amdgcn_readfirstlane(got);
            if (got < 0) break;
        }
        RV_WSYNC();
        const FrameM *f = &cur[wv];
        have = false;
        const int S = __builtin_amdgcn_readfirstlane((int)f->start), E = S + __builtin_amdgcn_readfirstlane((int)f->len);
        const int depth = __builtin_amdgcn_readfirstlane((int)f->depth), b = __builtin_amdgcn_readfirstlane((int)f->buf);
        const u32 myb = lane < KM ? (u32)f->b[sl] : 0u, mye = lane < KM ? (u32)f->e[sl] : 0u;      // lane s: the interval of sample s
        const int gb = (int)f->b[sl], ge = (int)f->e[sl];                                           // lane: the interval of sample lane & (KM - 1) (the chain's groups)
        const bool lv = myb < mye;
        const u64 live = __ballot(lv);
        const int ns = (int)__popcll(live);
        uint16_t *cs = sa2[b], *nsa = sa2[b ^ 1];
        uint16_t *cl = lc2[b], *nl_ = lc2[b ^ 1];
        uint8_t *cb = bw2[b], *nb = bw2[b ^ 1];
        MultiLeafStage<KM> st;
        st.cs = cs; st.smp = smp; st.seqb = seqb; st.la = eA + S; st.lb = eB + S; st.aux = act + S; st.skey = nsa + S;
        st.cme = cme[wv]; st.cpr = &cpr[wv][0][0]; st.wscore = C.wscore; st.wpen = C.wpen; st.model = C.gcmodel;
        if (lane == 0) { my_steps++; if ((u32)depth > my_maxdepth) my_maxdepth = (u32)depth; }

        // the windows that close at rank u, by descending l
        auto walk = [&](int u, auto &&emit) {
            if (u <= S || u >= E) return;
            const u32 nxt = (u + 1 < E) ? (u32)cl[u + 1] : 0u;
            const uint8_t sb0 = smp[cs[u]];
            if (sb0 & SMP_SEP) return;
            cen_t seen = (cen_t)1 << (sb0 & SMP_ID); u32 l = INF;
            uint8_t cnext = cb[u];
            bool lm = false;
            for (int k = 2; k <= ns; k++) {
                const int r = u - k + 1;
                if (r < S) break;
                const u32 v = cl[r + 1];
                l = v < l ? v : l;
                if (l < need || l <= nxt) break;
                const uint8_t sb = smp[cs[r]];
                const cen_t bit = (cen_t)1 << (sb & SMP_ID);
                if ((sb & SMP_SEP) || (seen & bit)) break;
                seen |= bit;
                const uint8_t c = cb[r];
                lm |= c != cnext || c == 'N' || c == '$' || is_lower_c(c);
                cnext = c;
                if (k >= nmin && lm && (r == S || (u32)cl[r] < l)) emit(r, k, (int)l, seen);
            }
        };

        // ---- the pick stage -> picked, the match P and its sample set -------------------------------------------------------
        bool picked = false;
        RvMtK P = RvMtK();
        cen_t setmask = 0;
        do {
            if (ns < 2 || ns < minn) break;
            // collect
            int m = 0, nfull = 0;
            for (int base = S; base < E; base += 64) {
                int cnt = 0;
                walk(base + lane, [&](int, int, int, cen_t) { cnt++; });
                const u32 inc = rv_wave_incl_sum_u32((u32)cnt);
                int at = m + (int)(inc - (u32)cnt), full = 0;
                walk(base + lane, [&](int r, int k, int l, cen_t seen) {
                    RvMtK c; c.l = l; c.row = r; c.sh = 0; c.n = k;
                    if (at < E - S) { st.putA(at, c); st.putSet(at, seen); }
                    at++;
                    full += k == ns ? 1 : 0;
                });
                m += __builtin_amdgcn_readlane((int)inc, 63);
                nfull += __builtin_amdgcn_readlane((int)rv_wave_incl_sum_u32((u32)full), 63);
            }
            if (m == 0) break;
            if (m >= E - S) { if (lane == 0) atomicOr(jflag, 2u); break; }      // (cannot happen: fewer inner nodes than ranks)
            // set, trim, chain, split (rv_chain_stage.h)
            const int res = rv_chain_stage_multi<KM>(st, lane, m, nfull, ns, live, gb - 1, ge, P, setmask);
            if (res > 0 && lane == 0) atomicOr(jflag, (u32)res);
            picked = res == RV_STAGE_PICK;
        } while (0);
        if (!picked) {
            if (lane == 0) atomicSub(&s_pending, 1);
            continue;
        }
        const u32 L = (u32)P.l;
        const int pn = P.n;
        u32 mem = 0;                                   // lane q < pn: member q, in member order
        if (lane < pn) { const u32 p = cs[P.row + lane]; mem = p + (u32)P.sh; wm[wv][smp[p] & SMP_ID] = (uint16_t)mem; }
        RV_WSYNC();
        const bool inset = lane < KM && ((setmask >> lane) & 1u);
        const u32 myp = wm[wv][sl];
        if (inset && (!lv || myp < myb || myp + L > mye)) atomicOr(A.err, 8u);
        // ---- the anchor: members in member order -----------------------------------------------------------------------------
        {
            u32 old = 0;
            if (lane == 0) { my_splits++; my_bp += L; old = atomicAdd(&s_cnt, (1u << 16) | (u32)pn); }
            old = (u32)__builtin_amdgcn_readfirstlane((int)old);
            const u32 slot = old >> 16, mo = old & 0xFFFFu;
            if (slot < acap) {
                if (lane == 0) { an_l[slot] = (uint16_t)L; an_n[slot] = (uint16_t)pn; an_mo[slot] = (uint16_t)mo; }
                if (lane < pn) an_pp[mo + lane] = (uint16_t)mem;
            } else {
                if (lane == 0 && slot == acap) s_nm_staged = mo;
                u32 ghi = 0, glo = 0;
                if (lane == 0) { const unsigned long long g = atomicAdd(A.count, (1ull << 32) | (unsigned long long)pn); ghi = (u32)(g >> 32); glo = (u32)g; }
                ghi = (u32)__builtin_amdgcn_readfirstlane((int)ghi); glo = (u32)__builtin_amdgcn_readfirstlane((int)glo);
                if (ghi < A.anchor_cap && glo + (u32)pn <= A.member_cap) {
                    if (lane == 0) { RvLeafMultiAnchor an; an.l = L; an.job = blockIdx.x; an.n = (u32)pn; an.moff = glo; A.anchors[ghi] = an; }
                    if (lane < pn) A.an_pos[(size_t)glo + lane] = (uint16_t)mem;
                } else if (lane == 0) atomicOr(A.err, 32u);
            }
        }
        for (cen_t mm = setmask; mm; mm &= mm - 1) {
            const u32 Pm = wm[wv][rv_cen_first(mm)];
            for (u32 j = lane; j < L; j += 64) if (Pm + j < (u32)n) smp[Pm + j] |= SMP_DONE;
        }
        // ---- graphalign, linear interval model: lead / trail on the set's samples, rest = the other live samples, whole -------
        const bool ll = inset && lv && myp > myb, tl = inset && lv && mye > myp + L, rl = lv && !inset;
        const u64 lmask = __ballot(ll);
        const u32 nlead = (u32)__builtin_amdgcn_readlane((int)rv_wave_incl_sum_u32(ll ? myp - myb : 0u), 63);
        const u32 ntrail = (u32)__builtin_amdgcn_readlane((int)rv_wave_incl_sum_u32(tl ? mye - myp - L : 0u), 63);
        const u32 nrest = (u32)__builtin_amdgcn_readlane((int)rv_wave_incl_sum_u32(rl ? mye - myb : 0u), 63);
        if (nlead + ntrail + nrest > (u32)(E - S)) { if (lane == 0) atomicOr(A.err, 8u); if (lane == 0) atomicSub(&s_pending, 1); continue; }
        // ---- label + split into the other copy: lead at S, trail behind it, rest behind that (four ranks per lane) ----------
        u32 cnt0 = 0, cnt1 = 0, cnt2 = 0;
        MinSt3 car; car.has = 0; car.v0 = INF; car.v1 = INF; car.v2 = INF;
        const u32 off1 = nlead, off2 = nlead + ntrail;
        for (int base = S; base < E; base += 4 * 64) {
            const int i0 = base + 4 * lane;
            u32 ev[4]; uint16_t pos[4]; uint8_t bo[4]; u32 cls = 0;      // cls: two bits per rank (1 = lead, 2 = trail, 3 = rest)
            MinSt3 agg; agg.has = 0; agg.v0 = INF; agg.v1 = INF; agg.v2 = INF;
            u32 n012 = 0;                                                // counts of this lane: ten bits each
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int i = i0 + r;
                u32 c = 0; ev[r] = INF; pos[r] = 0; bo[r] = 0;
                if (i < E) {
                    pos[r] = cs[i]; bo[r] = cb[i];
                    const u32 p = pos[r]; const uint8_t sb = smp[p];
                    if (!(sb & SMP_SEP)) {
                        const u32 s = sb & SMP_ID;
                        if ((setmask >> s) & 1u) {
                            const u32 mt = wm[wv][s];
                            c = p < mt ? 1u : (p >= mt + L ? 2u : 0u);
                            if (p == mt + L && bo[r] >= 'A' && bo[r] <= 'Z') bo[r] += 32;      // its left neighbour was just matched
                        } else c = 3u;
                    }
                    ev[r] = (i > S) ? (u32)cl[i] : INF;
                }
                cls |= c << (2 * r);
                n012 += (c == 1 ? 1u : 0u) + (c == 2 ? (1u << 10) : 0u) + (c == 3 ? (1u << 20) : 0u);
                agg.has |= c == 3 ? 4u : c;
                agg.v0 = c == 1 ? INF : (agg.v0 < ev[r] ? agg.v0 : ev[r]);
                agg.v1 = c == 2 ? INF : (agg.v1 < ev[r] ? agg.v1 : ev[r]);
                agg.v2 = c == 3 ? INF : (agg.v2 < ev[r] ? agg.v2 : ev[r]);
            }
            const MinSt3 inc = wave_incl_ms3(agg);
            const u32 ninc = rv_wave_incl_sum_u32(n012);
            MinSt3 x; x.has = from_lane_below(inc.has, 0u); x.v0 = from_lane_below(inc.v0, INF); x.v1 = from_lane_below(inc.v1, INF); x.v2 = from_lane_below(inc.v2, INF);
            x = ms3_combine(car, x);                   // the state in front of this lane's first rank
            const u32 nb4 = ninc - n012;
            u32 e0 = cnt0 + (nb4 & 0x3FFu), e1 = cnt1 + ((nb4 >> 10) & 0x3FFu), e2 = cnt2 + (nb4 >> 20);
            u32 r0 = x.v0, r1 = x.v1, r2 = x.v2;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const u32 c = (cls >> (2 * r)) & 3u;
                if (c == 1) {
                    const u32 v = r0 < ev[r] ? r0 : ev[r];
                    if (e0 < nlead) { nsa[S + e0] = pos[r]; nl_[S + e0] = (uint16_t)(e0 == 0 ? 0u : v); nb[S + e0] = bo[r]; }
                    e0++;
                } else if (c == 2) {
                    const u32 v = r1 < ev[r] ? r1 : ev[r];
                    if (e1 < ntrail) { nsa[S + off1 + e1] = pos[r]; nl_[S + off1 + e1] = (uint16_t)(e1 == 0 ? 0u : v); nb[S + off1 + e1] = bo[r]; }
                    e1++;
                } else if (c == 3) {
                    const u32 v = r2 < ev[r] ? r2 : ev[r];
                    if (e2 < nrest) { nsa[S + off2 + e2] = pos[r]; nl_[S + off2 + e2] = (uint16_t)(e2 == 0 ? 0u : v); nb[S + off2 + e2] = bo[r]; }
                    e2++;
                }
                r0 = c == 1 ? INF : (r0 < ev[r] ? r0 : ev[r]);
                r1 = c == 2 ? INF : (r1 < ev[r] ? r1 : ev[r]);
                r2 = c == 3 ? INF : (r2 < ev[r] ? r2 : ev[r]);
            }
            const u32 ntot = (u32)__builtin_amdgcn_readlane((int)ninc, 63);
            cnt0 += ntot & 0x3FFu; cnt1 += (ntot >> 10) & 0x3FFu; cnt2 += ntot >> 20;
            MinSt3 tot; tot.has = (u32)__builtin_amdgcn_readlane((int)inc.has, 63); tot.v0 = (u32)__builtin_amdgcn_readlane((int)inc.v0, 63);
            tot.v1 = (u32)__builtin_amdgcn_readlane((int)inc.v1, 63); tot.v2 = (u32)__builtin_amdgcn_readlane((int)inc.v2, 63);
            car = ms3_combine(car, tot);
        }
        RV_WSYNC();
        const int nl = (int)nlead, ntr = (int)ntrail, nrs = (int)nrest;
        if (lane == 0 && (cnt0 != nlead || cnt1 != ntrail || cnt2 != nrest)) atomicOr(A.err, 8u);      // (a sub-index that is not the suffixes of its intervals)
        const int cdepth = depth + 1;
        // a child is visited when at least max(2, minn) of its samples can hold a match; otherwise it counts as visited, not scanned
        bool dov[3];
        {
            const int longl = (int)__popcll(__ballot(ll && myp - myb >= need)), longt = (int)__popcll(__ballot(tl && mye - myp - L >= need));
            const int longr = (int)__popcll(__ballot(rl && mye - myb >= need));
            dov[0] = nl > 0 && longl >= nmin; dov[1] = ntr > 0 && longt >= nmin; dov[2] = nrs > 0 && longr >= nmin;
            const int skipped = (nl > 0 && !dov[0] ? 1 : 0) + (ntr > 0 && !dov[1] ? 1 : 0) + (nrs > 0 && !dov[2] ? 1 : 0);
            if (skipped && lane == 0) { my_steps += (u32)skipped; if ((u32)cdepth > my_maxdepth) my_maxdepth = (u32)cdepth; }
        }
        // ---- bubble_sort on the leading child: a cut at the match start of every sample with a leading interval, ascending ----
        for (u64 mm = dov[0] ? lmask : 0ull; mm; mm &= mm - 1) {
            const int s = (int)__builtin_ctzll(mm);
            const int B = (int)wm[wv][s], ib = (int)f->b[s];
            u32 nact = 0;
            for (int base = 0; base < nl; base += 64) {
                const int e = base + lane;
                bool on = false;
                if (e < nl) {
                    const int p = (int)nsa[S + e];
                    if (p >= ib && p < B) {
                        const int l0 = (int)nl_[S + e], l1 = (e + 1 < nl) ? (int)nl_[S + e + 1] : 0;
                        on = p + l0 > B || p + l1 > B;
                    }
                }
                const u64 mask = __ballot(on);
                if (on) act[S + nact + rv_lanes_below(mask)] = (uint16_t)e;
                nact += (u32)__popcll(mask);
            }
            RV_WSYNC();
            for (u32 ai = 0; ai < nact; ai++) {
                const int e = (int)act[S + ai];
                const int p = (int)nsa[S + e], l0 = (int)nl_[S + e];
                if (p < B && p + l0 > B) {
                    const int t = B - p; const uint8_t tB = nb[S + e];
                    int x = 0;
                    for (int hi = e;; hi -= 64) {
                        const int r = hi - lane;
                        const u64 mask = __ballot(r >= 0 && (r == 0 || (int)nl_[S + r] < t));
                        if (mask) { x = hi - (int)__builtin_ctzll(mask); break; }
                    }
                    const u32 lnext = (e < nl - 1) ? (u32)nl_[S + e + 1] : 0u;
                    for (int hi = e; hi > x; hi -= 64) {
                        const int r = hi - lane;
                        uint16_t vs = 0, vl = 0; uint8_t vb = 0;
                        if (r > x) { vs = nsa[S + r - 1]; vl = nl_[S + r - 1]; vb = nb[S + r - 1]; }
                        RV_WSYNC();
                        if (r > x) { nsa[S + r] = vs; nl_[S + r] = vl; nb[S + r] = vb; }
                        RV_WSYNC();
                    }
                    if (lane == 0) {
                        nsa[S + x] = (uint16_t)p; nb[S + x] = tB;
                        if (x + 1 < nl) nl_[S + x + 1] = (uint16_t)t;
                        if (e < nl - 1 && (u32)l0 < lnext) nl_[S + e + 1] = (uint16_t)l0;
                    }
                } else if (e < nl - 1) {
                    const int l1 = (int)nl_[S + e + 1];
                    if (lane == 0 && p < B && p + l1 > B && l1 > l0) nl_[S + e + 1] = (uint16_t)(B - p);
                }
                RV_WSYNC();
            }
        }
        // ---- children: this wave goes on with the smallest one, the others go to the stack for any wave ----------------------
        const int cstart[3] = {S, S + nl, S + nl + ntr}, clen[3] = {nl, ntr, nrs};
        const uint16_t cbeg[3] = {(uint16_t)(ll ? myb : 0u), (uint16_t)(tl ? myp + L : 0u), (uint16_t)(rl ? myb : 0u)};
        const uint16_t cend[3] = {(uint16_t)(ll ? myp : 0u), (uint16_t)(tl ? mye : 0u), (uint16_t)(rl ? mye : 0u)};
        int keepc = -1, keeplen = LN + 1;
#pragma unroll
        for (int c = 0; c < 3; c++) if (dov[c] && clen[c] < keeplen) { keepc = c; keeplen = clen[c]; }
        const int npush = (dov[0] ? 1 : 0) + (dov[1] ? 1 : 0) + (dov[2] ? 1 : 0) - (keepc >= 0 ? 1 : 0);
        if (npush > 0) {
            int t = -1;
            if (lane == 0) {
                while (atomicCAS(&s_lock, 0, 1) != 0) __builtin_amdgcn_s_sleep(1);
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                t = s_top;
                if (t + npush <= MAXSTACK) { s_top = t + npush; atomicAdd(&s_pending, npush); }
                else { atomicOr(jflag, 32u); t = -1; }      // (the job finishes on the host; the children that found no room are left out)
            }
            t = __builtin_amdgcn_readfirstlane(t);
            if (t >= 0) {                              // the lock is held until the frames are written
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    if (!dov[c] || c == keepc) continue;
                    FrameM *o = &stack[t++];
                    if (lane == 0) { o->start = (uint16_t)cstart[c]; o->len = (uint16_t)clen[c]; o->depth = (uint16_t)cdepth; o->buf = (uint16_t)(b ^ 1); }
                    if (lane < KM) { o->b[lane] = cbeg[c]; o->e[lane] = cend[c]; }
                }
            }
            RV_WSYNC();
            if (lane == 0) { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); atomicExch(&s_lock, 0); }
        }
        if (keepc >= 0) {
            FrameM *o = &cur[wv];
            uint16_t kb = 0, ke = 0; int ks = 0, kl = 0;
#pragma unroll
            for (int c = 0; c < 3; c++) if (c == keepc) { kb = cbeg[c]; ke = cend[c]; ks = cstart[c]; kl = clen[c]; }
            RV_WSYNC();
            if (lane == 0) { o->start = (uint16_t)ks; o->len = (uint16_t)kl; o->depth = (uint16_t)cdepth; o->buf = (uint16_t)(b ^ 1); }
            if (lane < KM) { o->b[lane] = kb; o->e[lane] = ke; }
        } else if (lane == 0) {
            atomicSub(&s_pending, 1);
        }
        have = keepc >= 0;
    }
    if (lane == 0) {
        atomicAdd(&s_stats[0], (unsigned long long)my_steps); atomicAdd(&s_stats[1], (unsigned long long)my_splits);
        atomicAdd(&s_stats[2], (unsigned long long)my_bp); atomicMax(&s_stats[3], (unsigned long long)my_maxdepth);
    }
    __syncthreads();                                   // every wave has left the loop: the job is finished
    const u32 na_all = s_cnt >> 16;
    const u32 na = na_all < acap ? na_all : acap, nm = na_all <= acap ? (s_cnt & 0xFFFFu) : s_nm_staged;
    if (tid == 0) {
        s_base = na ? atomicAdd(A.count, ((unsigned long long)na << 32) | (unsigned long long)nm) : 0ull;
        atomicAdd(&A.stats[0], s_stats[0]); atomicAdd(&A.stats[1], s_stats[1]); atomicAdd(&A.stats[2], s_stats[2]); atomicMax(&A.stats[3], s_stats[3]);
    }
    __syncthreads();
    if (na) {
        const u32 ba = (u32)(s_base >> 32), bm = (u32)s_base;
        if (ba + na <= A.anchor_cap && bm + nm <= A.member_cap && nm <= (u32)LN) {
            for (u32 k = tid; k < na; k += NT) { RvLeafMultiAnchor an; an.l = an_l[k]; an.job = blockIdx.x; an.n = an_n[k]; an.moff = bm + an_mo[k]; A.anchors[ba + k] = an; }
            for (u32 k = tid; k < nm; k += NT) A.an_pos[(size_t)bm + k] = an_pp[k];
        } else if (tid == 0) atomicOr(A.err, 32u);
    }
    for (int i = tid; i < n; i += NT) {
        if (smp[i] & SMP_DONE) { const uint8_t ch = A.T[job.beg + i]; if (ch >= 'A' && ch <= 'Z') A.T[job.beg + i] = ch + 32; }
    }
}

}  // namespace

int rv_leaf_multi_chain_launch(hipStream_t q, const RvLeafMultiArgs &a, const RvLeafMultiChainArgs &c, int njobs, int kmax) {
    if (njobs <= 0) return 0;
    if (!c.flags || c.wscore < 0 || c.wpen < 0 || c.wscore > RV_LEAF_MCHAIN_WMAX || c.wpen > RV_LEAF_MCHAIN_WMAX || c.gcmodel < 0 || c.gcmodel > 2 || a.minl < 1) {
        rv_set_error("rv_leaf_multi_chain_launch: arguments the chain form of the multi-sample leaf kernel does not take");
        return -1;
    }
    if (kmax == RV_MANY_KMAX) hipLaunchKernelGGL(k_leaf_multi_chain<RV_MANY_KMAX>, dim3((unsigned)njobs), dim3(NT), 0, q, a, c);
    else if (kmax == RV_MANY_WIDE_KMAX) hipLaunchKernelGGL(k_leaf_multi_chain<RV_MANY_WIDE_KMAX>, dim3((unsigned)njobs), dim3(NT), 0, q, a, c);
    else { rv_set_error("rv_leaf_multi_chain_launch: the kernel has forms for %d and %d samples, not %d", RV_MANY_KMAX, RV_MANY_WIDE_KMAX, kmax); return -1; }
    RV_LAUNCH_CHECK();
    return 0;
}
