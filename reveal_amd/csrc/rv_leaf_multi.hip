// rv_leaf_multi.hip -- the whole recursion of a job of 3 .. RV_MANY_KMAX samples inside one workgroup (rv_many.hip, RV_MANY_MULTI), and in its
// wide form of a job of up to RV_MANY_WIDE_KMAX = 64 samples (RV_MANY_WIDE: the jobs of 17 .. 64 sequences).
//
// k_leaf (rv_leaf.hip) with one interval per SAMPLE in a frame instead of two: one workgroup per job, the arrays in LDS in two
// copies, one wavefront per sub-index, the waves taking sub-indices from a shared stack.  A job is `s0$s1$..s(k-1)$`, at most
// RV_LEAF_N ranks and contiguous in the round's text, so positions and LCP values are job-local and 16 bits wide.
//   sample  a byte per local position (the number of '$' in front of it), counted once when the job is loaded; bit 6 marks the
//           '$' themselves (suffixes no child holds), bit 7 what an anchor covered -- the text is lower-cased from it at the end
//   scan    the matches the benchmark picker can take (oracle/reveal_oracle.c ro_getmultimums + ro_bench_picker; reveal.c:436-580,
//           227-259): LCP intervals of exactly ns ranks, ns = the non-empty intervals of the sub-index -- a window predicate per rank
//   pick    the longest, ties -> the smallest member position
//   split   lead = what lies in front of the match on every sample, trail = what lies behind it; a rank's class follows from the
//           member position of its own sample.  Running-minimum LCP per child (reveal.c:582-664)
//   bubble  bubble_sort on the leading child, one cut per sample with a leading interval, ascending (reveal.c:666-727)
// Every sub-index of such a job takes this path, also once it is down to two samples (scan_index decides by the main index).
//
// The kernel is a template over the sample bound KM.  Lane s of a wavefront owns sample s (64-bit ballots), the sample id lies in the low bits
// of the `smp` byte below SMP_SEP (0x40), and the scan's census has a bit per sample: 64 is the bound of all three, and of the one-word
// census of the level pipeline's multi-sample scan (rv_scan.hip) that finishes such jobs above RV_LEAF_N ranks.  Wider jobs stay ordinary.
//   KM = 16   FrameM 72 B, a 32-bit census, 39 664 B of LDS per workgroup: the code, the footprint and the results it had before the template
//   KM = 64   FrameM 264 B (96 stack + 4 current frames: 26 400 B), a 64-bit census, arrays 32 256 B, the picked members 512 B: 59 248 B of
//             LDS per workgroup (compiler remark, gfx950; a workgroup may declare 160 KiB): two workgroups per CU; 103 VGPRs, no scratch
// MAXSTACK does not depend on KM: the frames that wait are O(waves x log n), n <= RV_LEAF_N ranks whatever the number of samples.
#include "rv_leaf_multi.h"

namespace {

constexpr int NT = 256;
constexpr int LN = RV_LEAF_N;
constexpr int NW = NT / 64;
constexpr int MAXSTACK = 96;             // frames waiting for a wave: O(waves x log n), a wave goes on with the smaller child
constexpr int ACAP = 256;            // anchors staged per workgroup; their members (at most LN: anchors cover disjoint text) all fit
constexpr u32 INF = 0xFFFFFFFFu;
constexpr uint8_t SMP_SEP = 0x40, SMP_DONE = 0x80;      // (the sample id lies below them: KM - 1, at most six bits)
static_assert(LN <= 2048, "positions in 16 bits, 8 per thread when a job is loaded");

template <int KM>
struct FrameMT { uint16_t start, len, depth, buf; uint16_t b[KM], e[KM]; };      // interval [b, e) of every sample, job-local; empty: b >= e
template <int KM> struct Census { typedef u32 type; };      // a bit per sample of the window the scan looks at
template <> struct Census<RV_MANY_WIDE_KMAX> { typedef u64 type; };


__device__ inline bool is_lower_c(uint8_t c) { return c >= 'a' && c <= 'z'; }
__device__ inline u32 from_lane_below(u32 x, u32 first) { return (u32)__builtin_amdgcn_update_dpp((int)first, (int)x, 0x138 /* wave_shr:1 */, 0xf, 0xf, false); }

// running minimum of the LCP values since the last rank of the leading / trailing child (rv_leaf.hip MinSt2)
struct MinSt2 { u32 has, v0, v1; };
__device__ inline MinSt2 ms2_combine(MinSt2 a, MinSt2 b) {      // a, then b
    MinSt2 r; r.has = a.has | b.has;
    r.v0 = (b.has & 1u) ? b.v0 : (a.v0 < b.v0 ? a.v0 : b.v0);
    r.v1 = (b.has & 2u) ? b.v1 : (a.v1 < b.v1 ? a.v1 : b.v1);
    return r;
}
__device__ inline MinSt2 wave_incl_ms2(MinSt2 m) {
    const int lane = threadIdx.x & 63;
#define LM_STEP_(CTRL, RM, TAKE) {                                                                                    \
        MinSt2 t; t.has = rv_dpp_u32<CTRL, RM>(m.has); t.v0 = rv_dpp_u32<CTRL, RM>(m.v0); t.v1 = rv_dpp_u32<CTRL, RM>(m.v1);    \
        const MinSt2 c = ms2_combine(t, m);                                                                           \
        if (TAKE) m = c;                                                                                              \
    }
    RV_WAVE_SCAN_STEPS(LM_STEP_)
#undef LM_STEP_
    return m;
}

// KM: the sample bound of the form, RV_MANY_KMAX (16) or RV_MANY_WIDE_KMAX (64) -- a power of two and at most a wavefront's lanes
template <int KM>
__global__ __launch_bounds__(NT) void k_leaf_multi(RvLeafMultiArgs A) {
    static_assert(KM == RV_MANY_KMAX || KM == RV_MANY_WIDE_KMAX, "the sample in KM - 1 <= 0x3F of the smp byte, lane s owns sample s");
    static_assert((KM & (KM - 1)) == 0 && KM <= 64 && KM - 1 < SMP_SEP && KM <= NT, "lane & (KM - 1), 64-bit ballots, tid < KM");
    constexpr uint8_t SMP_ID = (uint8_t)(KM - 1);
    typedef typename Census<KM>::type cen_t;
    typedef FrameMT<KM> FrameM;
    __shared__ uint16_t sa2[2][LN], lc2[2][LN];
    __shared__ uint8_t bw2[2][LN];
    __shared__ uint8_t smp[LN];
    __shared__ uint16_t act[LN];
    __shared__ FrameM stack[MAXSTACK];
    __shared__ FrameM cur[NW];
    __shared__ uint16_t wm[NW][KM];               // the picked match: its member on every sample
    __shared__ uint16_t an_l[ACAP], an_n[ACAP], an_mo[ACAP], an_pp[LN];      // staged anchors: length, members, first member in an_pp
    __shared__ int s_top, s_pending, s_lock, s_bad;
    __shared__ u32 s_cnt, s_nm_staged, s_part[NW];                           // s_cnt: anchors << 16 | members
    __shared__ unsigned long long s_base;
    __shared__ unsigned long long s_stats[4];

    const RvLeafMultiJob job = A.jobs[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n = job.n;
    if (n < 2 || n > LN) { if (tid == 0) atomicOr(A.err, 16u); return; }
    for (int i = tid; i < n; i += NT) {
        sa2[0][i] = (uint16_t)((int64_t)A.SA[job.beg + i] - job.beg); lc2[0][i] = (uint16_t)A.LCP[job.beg + i]; bw2[0][i] = A.BWT[job.beg + i] & RV_BWT_CHAR;
    }
    // the sample of every position: a thread takes eight consecutive ones and counts the '$' in front of them
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
                if (p == n - 1) bad = true;            // (the text of a job ends with '$')
            }
        }
        if (bad) { s_bad = 1; }
    }
    __syncthreads();                                   // the last workgroup barrier in front of the recursion
    if (s_bad) { if (tid == 0) atomicOr(A.err, 16u); return; }

    const u32 need = A.minl > 1 ? (u32)A.minl : 1u;
    const int minn = A.minn;
    const u32 acap = A.stage_cap < (u32)ACAP ? A.stage_cap : (u32)ACAP;
    u32 my_steps = 0, my_splits = 0, my_maxdepth = 0; u64 my_bp = 0;     // accumulated by lane 0 of every wave
    bool have = wv == 0;

    for (;;) {
        if (!have) {
            // take a sub-index from the shared stack, or leave once every sub-index of the job is finished
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
        const u32 myb = lane < KM ? (u32)f->b[lane & (KM - 1)] : 0u, mye = lane < KM ? (u32)f->e[lane & (KM - 1)] : 0u;      // lane s: the interval of sample s
        const u64 live = __ballot(myb < mye);
        const int ns = (int)__popcll(live);            // nsamples of the sub-index (reveal.c:1028-1042)
        const bool lv = myb < mye;
        uint16_t *cs = sa2[b], *nsa = sa2[b ^ 1];
        uint16_t *cl = lc2[b], *nl_ = lc2[b ^ 1];
        uint8_t *cb = bw2[b], *nb = bw2[b ^ 1];
        if (lane == 0) { my_steps++; if ((u32)depth > my_maxdepth) my_maxdepth = (u32)depth; }

        // ---- scan + picker: the LCP intervals of exactly ns ranks, every member from another sample ------------------------
        u64 best = 0;
        if (ns >= 2 && ns >= minn) {
            for (int i = S + lane; i + ns <= E; i += 64) {
                u32 l = INF;
                for (int j = 1; j < ns; j++) { const u32 v = cl[i + j]; l = v < l ? v : l; }
                if (l < need) continue;
                if (i > S && (u32)cl[i] >= l) continue;
                if (i + ns < E && (u32)cl[i + ns] >= l) continue;
                cen_t seen = 0; u32 minp = 0xFFFFu; bool dup = false, lm = false; uint8_t cprev = 0;
                for (int j = 0; j < ns; j++) {
                    const u32 p = cs[i + j]; const uint8_t sb = smp[p], c = cb[i + j];
                    const cen_t bit = (cen_t)1 << (sb & SMP_ID);
                    dup |= (seen & bit) != 0 || (sb & SMP_SEP) != 0;
                    seen |= bit;
                    minp = p < minp ? p : minp;
                    if (j > 0) lm |= cprev != c || cprev == 'N' || cprev == '$' || is_lower_c(cprev);      // (position 0 has '$' in front: reveal.c:241-243)
                    cprev = c;
                }
                if (dup || !lm) continue;
                const u64 key = ((u64)l << 32) | ((u64)(0xFFFFu - minp) << 16) | (u64)(u32)i;      // longest, then smallest position; the first rank rides along
                best = key > best ? key : best;
            }
        }
        best = rv_wave_max_u64(best);
        if (best == 0) {
            if (lane == 0) atomicSub(&s_pending, 1);
            continue;
        }
        const u32 L = (u32)(best >> 32);
        const int lb = (int)(best & 0xFFFFu);
        if (lane < ns) { const u32 p = cs[lb + lane]; wm[wv][smp[p] & SMP_ID] = (uint16_t)p; }
        RV_WSYNC();
        const u32 myp = wm[wv][lane & (KM - 1)];       // the member on this lane's sample (lanes with an interval)
        if (lv && (myp < myb || myp + L > mye)) atomicOr(A.err, 8u);
        // ---- the anchor: members ascending = in sample order ---------------------------------------------------------------
        {
            u32 old = 0;
            if (lane == 0) { my_splits++; my_bp += L; old = atomicAdd(&s_cnt, (1u << 16) | (u32)ns); }
            old = (u32)__builtin_amdgcn_readfirstlane((int)old);
            const u32 slot = old >> 16, mo = old & 0xFFFFu, r = (u32)__popcll(live & ((1ull << lane) - 1ull));
            if (slot < acap) {
                if (lane == 0) { an_l[slot] = (uint16_t)L; an_n[slot] = (uint16_t)ns; an_mo[slot] = (uint16_t)mo; }
                if (lv) an_pp[mo + r] = (uint16_t)myp;
            } else {                                   // (more anchors than the staging holds: minl of a few bases)
                if (lane == 0 && slot == acap) s_nm_staged = mo;
                u32 ghi = 0, glo = 0;
                if (lane == 0) { const unsigned long long g = atomicAdd(A.count, (1ull << 32) | (unsigned long long)ns); ghi = (u32)(g >> 32); glo = (u32)g; }
                ghi = (u32)__builtin_amdgcn_readfirstlane((int)ghi); glo = (u32)__builtin_amdgcn_readfirstlane((int)glo);
                if (ghi < A.anchor_cap && glo + (u32)ns <= A.member_cap) {
                    if (lane == 0) { RvLeafMultiAnchor an; an.l = L; an.job = blockIdx.x; an.n = (u32)ns; an.moff = glo; A.anchors[ghi] = an; }
                    if (lv) A.an_pos[(size_t)glo + r] = (uint16_t)myp;
                } else if (lane == 0) atomicOr(A.err, 32u);
            }
        }
        for (u64 mm = live; mm; mm &= mm - 1) {        // what the match covers is lower-cased when the job ends
            const u32 P = wm[wv][__builtin_ctzll(mm)];
            for (u32 j = lane; j < L; j += 64) smp[P + j] |= SMP_DONE;
        }
        // ---- graphalign: lead [myb, myp), trail [myp + L, mye) on every sample; no rest ------------------------------------
        const bool ll = lv && myp > myb, tl = lv && mye > myp + L;
        const u64 lmask = __ballot(ll), tmask = __ballot(tl);
        const u32 sizes = (u32)__builtin_amdgcn_readlane((int)rv_wave_incl_sum_u32(lv ? ((myp - myb) | ((mye - myp - L) << 16)) : 0u), 63);
        const u32 nlead = sizes & 0xFFFFu, ntrail = sizes >> 16;
        // ---- label + split into the other copy: lead at S, trail right behind it (rv_leaf.hip; four ranks per lane) --------
        u32 cnt0 = 0, cnt1 = 0;
        MinSt2 car; car.has = 0; car.v0 = INF; car.v1 = INF;
        for (int base = S; base < E; base += 4 * 64) {
            const int i0 = base + 4 * lane;
            u32 ev[4]; uint16_t pos[4]; uint8_t bo[4]; u32 cls = 0;      // cls: two bits per rank (1 = lead, 2 = trail)
            MinSt2 agg; agg.has = 0; agg.v0 = INF; agg.v1 = INF;
            u32 n01 = 0;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int i = i0 + r;
                u32 c = 0; ev[r] = INF; pos[r] = 0; bo[r] = 0;
                if (i < E) {
                    pos[r] = cs[i]; bo[r] = cb[i];
                    const u32 p = pos[r]; const uint8_t sb = smp[p];
                    if (!(sb & SMP_SEP)) {
                        const u32 m = wm[wv][sb & SMP_ID];
                        c = p < m ? 1u : (p >= m + L ? 2u : 0u);
                        if (p == m + L && bo[r] >= 'A' && bo[r] <= 'Z') bo[r] += 32;      // its left neighbour was just matched
                    }
                    ev[r] = (i > S) ? (u32)cl[i] : INF;      // every rank is lead, trail, matched or a '$': no skipped updates
                }
                cls |= c << (2 * r);
                n01 += (c == 1 ? 1u : 0u) + (c == 2 ? 0x10000u : 0u);
                agg.has |= c;
                agg.v0 = c == 1 ? INF : (agg.v0 < ev[r] ? agg.v0 : ev[r]);
                agg.v1 = c == 2 ? INF : (agg.v1 < ev[r] ? agg.v1 : ev[r]);
            }
            const MinSt2 inc = wave_incl_ms2(agg);
            const u32 ninc = rv_wave_incl_sum_u32(n01);
            MinSt2 x; x.has = from_lane_below(inc.has, 0u); x.v0 = from_lane_below(inc.v0, INF); x.v1 = from_lane_below(inc.v1, INF);
            x = ms2_combine(car, x);                   // the state in front of this lane's first rank
            u32 e0 = cnt0 + ((ninc - n01) & 0xFFFFu), e1 = cnt1 + ((ninc - n01) >> 16);
            u32 r0 = x.v0, r1 = x.v1;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const u32 c = (cls >> (2 * r)) & 3u;
                if (c == 1) {
                    const u32 v = r0 < ev[r] ? r0 : ev[r];
                    if (e0 < nlead) { nsa[S + e0] = pos[r]; nl_[S + e0] = (uint16_t)(e0 == 0 ? 0u : v); nb[S + e0] = bo[r]; }
                    e0++;
                } else if (c == 2) {
                    const u32 v = r1 < ev[r] ? r1 : ev[r];
                    if (e1 < ntrail) { nsa[S + nlead + e1] = pos[r]; nl_[S + nlead + e1] = (uint16_t)(e1 == 0 ? 0u : v); nb[S + nlead + e1] = bo[r]; }
                    e1++;
                }
                r0 = c == 1 ? INF : (r0 < ev[r] ? r0 : ev[r]);
                r1 = c == 2 ? INF : (r1 < ev[r] ? r1 : ev[r]);
            }
            const u32 ntot = (u32)__builtin_amdgcn_readlane((int)ninc, 63);
            cnt0 += ntot & 0xFFFFu; cnt1 += ntot >> 16;
            MinSt2 tot; tot.has = (u32)__builtin_amdgcn_readlane((int)inc.has, 63); tot.v0 = (u32)__builtin_amdgcn_readlane((int)inc.v0, 63); tot.v1 = (u32)__builtin_amdgcn_readlane((int)inc.v1, 63);
            car = ms2_combine(car, tot);
        }
        RV_WSYNC();
        const int nl = (int)nlead, ntr = (int)ntrail;
        if (lane == 0 && (cnt0 != nlead || cnt1 != ntrail)) atomicOr(A.err, 8u);      // (a sub-index that is not the suffixes of its intervals)
        const int cdepth = depth + 1;
        bool do_lead = nl > 0, do_trail = ntr > 0;
        {
            // The picker takes a match on EVERY sample of a child: a child of fewer than two samples, of fewer than minn, or with
            // an interval shorter than the shortest match has nothing to pick (bubble_sort keeps every LCP value inside the
            // intervals): counted as visited, not scanned
            const int nsl = (int)__popcll(lmask), nst = (int)__popcll(tmask);
            const bool short_l = __ballot(ll && myp - myb < need) != 0, short_t = __ballot(tl && mye - myp - L < need) != 0;
            if (do_lead && (nsl < 2 || nsl < minn || short_l)) { do_lead = false; if (lane == 0) { my_steps++; if ((u32)cdepth > my_maxdepth) my_maxdepth = (u32)cdepth; } }
            if (do_trail && (nst < 2 || nst < minn || short_t)) { do_trail = false; if (lane == 0) { my_steps++; if ((u32)cdepth > my_maxdepth) my_maxdepth = (u32)cdepth; } }
        }
        // ---- bubble_sort on the leading child: a cut at the match start of every sample with a leading interval, ascending ----
        for (u64 mm = do_lead ? lmask : 0ull; mm; mm &= mm - 1) {
            const int s = (int)__builtin_ctzll(mm);
            const int B = (int)wm[wv][s], ib = (int)f->b[s];
            u32 nact = 0;                              // actives in rank order
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
                    int x = 0;                         // the largest r <= e with r == 0 or LCP[r] < t
                    for (int hi = e;; hi -= 64) {
                        const int r = hi - lane;
                        const u64 mask = __ballot(r >= 0 && (r == 0 || (int)nl_[S + r] < t));
                        if (mask) { x = hi - (int)__builtin_ctzll(mask); break; }
                    }
                    const u32 lnext = (e < nl - 1) ? (u32)nl_[S + e + 1] : 0u;
                    // shift [x, e-1] -> [x+1, e], from the top in pieces of 64: the wave reads before it writes
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
        // ---- children: this wave goes on with the smaller one, the larger one goes to the stack for any wave -------------------
        const bool keep_lead = do_lead && (!do_trail || nl <= ntr);
        const uint16_t lb_ = (uint16_t)(ll ? myb : 0u), le_ = (uint16_t)(ll ? myp : 0u), tb_ = (uint16_t)(tl ? myp + L : 0u), te_ = (uint16_t)(tl ? mye : 0u);
        if (do_lead && do_trail) {
            int t = -1;
            if (lane == 0) {
                while (atomicCAS(&s_lock, 0, 1) != 0) __builtin_amdgcn_s_sleep(1);
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                t = s_top;
                if (t < MAXSTACK) { s_top = t + 1; atomicAdd(&s_pending, 1); }
                else { atomicOr(A.err, 4u); t = -1; }
            }
            t = __builtin_amdgcn_readfirstlane(t);
            if (t >= 0) {                              // the other child; the lock is held until its frame is written
                FrameM *o = &stack[t];
                if (lane == 0) { o->start = (uint16_t)(keep_lead ? S + nl : S); o->len = (uint16_t)(keep_lead ? ntr : nl); o->depth = (uint16_t)cdepth; o->buf = (uint16_t)(b ^ 1); }
                if (lane < KM) { o->b[lane] = keep_lead ? tb_ : lb_; o->e[lane] = keep_lead ? te_ : le_; }
            }
            RV_WSYNC();
            if (lane == 0) { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); atomicExch(&s_lock, 0); }
        }
        if (do_lead || do_trail) {
            FrameM *o = &cur[wv];
            if (lane == 0) { o->start = (uint16_t)(keep_lead ? S : S + nl); o->len = (uint16_t)(keep_lead ? nl : ntr); o->depth = (uint16_t)cdepth; o->buf = (uint16_t)(b ^ 1); }
            if (lane < KM) { o->b[lane] = keep_lead ? lb_ : tb_; o->e[lane] = keep_lead ? le_ : te_; }
        } else if (lane == 0) {
            atomicSub(&s_pending, 1);
        }
        have = do_lead || do_trail;
    }
    if (lane == 0) {
        atomicAdd(&s_stats[0], (unsigned long long)my_steps); atomicAdd(&s_stats[1], (unsigned long long)my_splits);
        atomicAdd(&s_stats[2], (unsigned long long)my_bp); atomicMax(&s_stats[3], (unsigned long long)my_maxdepth);
    }
    __syncthreads();                                   // every wave has left the loop: the job is finished
    const u32 na_all = s_cnt >> 16;
    const u32 na = na_all < acap ? na_all : acap, nm = na_all <= acap ? (s_cnt & 0xFFFFu) : s_nm_staged;
    if (tid == 0) {
        s_base = na ? atomicAdd(A.count, ((unsigned long long)na << 32) | (unsigned long long)nm) : 0ull;      // ONE reservation per workgroup
        atomicAdd(&A.stats[0], s_stats[0]); atomicAdd(&A.stats[1], s_stats[1]); atomicAdd(&A.stats[2], s_stats[2]); atomicMax(&A.stats[3], s_stats[3]);
    }
    __syncthreads();
    if (na) {
        const u32 ba = (u32)(s_base >> 32), bm = (u32)s_base;
        if (ba + na <= A.anchor_cap && bm + nm <= A.member_cap) {
            for (u32 k = tid; k < na; k += NT) { RvLeafMultiAnchor an; an.l = an_l[k]; an.job = blockIdx.x; an.n = an_n[k]; an.moff = bm + an_mo[k]; A.anchors[ba + k] = an; }
            for (u32 k = tid; k < nm; k += NT) A.an_pos[(size_t)bm + k] = an_pp[k];
        } else if (tid == 0) atomicOr(A.err, 32u);
    }
    // the final text (reveal.c:1230-1234): lower case under every member of every anchor
    for (int i = tid; i < n; i += NT) {
        if (smp[i] & SMP_DONE) { const uint8_t ch = A.T[job.beg + i]; if (ch >= 'A' && ch <= 'Z') A.T[job.beg + i] = ch + 32; }
    }
}

}  // namespace

int rv_leaf_multi_launch(hipStream_t q, const RvLeafMultiArgs &a, int njobs, int kmax) {
    if (njobs <= 0) return 0;
    if (kmax == RV_MANY_KMAX) hipLaunchKernelGGL(k_leaf_multi<RV_MANY_KMAX>, dim3((unsigned)njobs), dim3(NT), 0, q, a);
    else if (kmax == RV_MANY_WIDE_KMAX) hipLaunchKernelGGL(k_leaf_multi<RV_MANY_WIDE_KMAX>, dim3((unsigned)njobs), dim3(NT), 0, q, a);
    else { rv_set_error("rv_leaf_multi_launch: no form of the kernel for %d samples", kmax); return -1; }
    RV_LAUNCH_CHECK();
    return 0;
}
