// rv_leaf_stages.h -- the leaf kernel's stages, shared by its two forms: k_leaf (rv_leaf.hip: the built-in picker) and k_leaf_chain
// (rv_leaf_chain.hip: the reference's default picker for two samples).  The frame stack, the split, bubble_sort and the anchor staging are
// ONE body (leaf_run) that is instantiated with a pick stage:
//   PICK::pick(A, P, X, L, pa, pb)   the decision for the sub-index X -> whether a match was chosen, and the match (length, member of sample 0 / 1)
//   PICK::fail(A, P, bits)           a sub-index that cannot be finished (stack overflow, ranks that do not match the intervals)
// P is the form's own argument block (nothing for the built-in picker).
#pragma once
#include "rv_common.h"
#include "rv_leaf.h"
#include <type_traits>

namespace {

constexpr int NT = 256;
constexpr int LN = RV_LEAF_N;
constexpr u32 INF = 0xFFFFFFFFu;
constexpr int NW = NT / 64;
constexpr int MAXSTACK = 128;
constexpr int ACAP = 256;            // anchors staged per workgroup (a root of 2048 ranks holds ~5 at minl 20)

typedef std::make_unsigned<sa_t>::type usa_t;      // positions compared in their own width (32 bits in reveallib)
struct Frame { int start, len, depth, buf; int64_t a0, a1, b0, b1; };   // sample-0 interval [a0,a1), sample-1 interval [b0,b1); empty if a0>=a1

__device__ inline bool is_lower_c(uint8_t c) { return c >= 'a' && c <= 'z'; }
__device__ inline bool left_maximal(uint8_t ca, uint8_t cb) { return (ca != cb) || ca == 'N' || ca == '$' || is_lower_c(ca); }

__device__ inline u64 hash_step(u64 acc, u64 i, int64_t v) {      // oracle/reveal_oracle.c ro_hash_step
    u64 x = (u64)v + (i + 1) * 0x9E3779B97F4A7C15ULL;
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ULL;
    x ^= x >> 27; x *= 0x94d049bb133111ebULL;
    x ^= x >> 31;
    return acc + x;
}

// ---- wave-level collectives (DPP, rv_common.h) ------------------------------------------
// Every sub-index is processed by ONE wavefront: no workgroup barrier inside the recursion, the four waves of a workgroup
// work on different sub-indices of the same root (disjoint rank ranges of the LDS arrays).

__device__ inline u64 wave_max_u64(u64 v) { return rv_wave_max_u64(v); }
__device__ inline u64 wave_sum_u64(u64 v) {       // trace mode only
    for (int d = 32; d >= 1; d >>= 1) v += ((u64)__shfl_xor((u32)(v >> 32), d, 64) << 32) | __shfl_xor((u32)v, d, 64);
    return v;
}
// the value of the lane below (lane 0: `first`)
__device__ inline u32 from_lane_below(u32 x, u32 first) { return (u32)__builtin_amdgcn_update_dpp((int)first, (int)x, 0x138 /* wave_shr:1 */, 0xf, 0xf, false); }

// Running minimum of the LCP values since the last rank of class 0 / class 1 (reveal.c:582-664 keeps one running minimum per
// child): has = bit k set once a rank of class k was seen, v[k] = minimum since then.  Inclusive scan over the wave.
struct MinSt2 { u32 has, v0, v1; };
__device__ inline MinSt2 ms2_combine(MinSt2 a, MinSt2 b) {      // a, then b
    MinSt2 r; r.has = a.has | b.has;
    r.v0 = (b.has & 1u) ? b.v0 : (a.v0 < b.v0 ? a.v0 : b.v0);
    r.v1 = (b.has & 2u) ? b.v1 : (a.v1 < b.v1 ? a.v1 : b.v1);
    return r;
}
__device__ inline MinSt2 wave_incl_ms2(MinSt2 m) {
    const int lane = threadIdx.x & 63;
#define LF_STEP_(CTRL, RM, TAKE) {                                                                                    \
        MinSt2 t; t.has = rv_dpp_u32<CTRL, RM>(m.has); t.v0 = rv_dpp_u32<CTRL, RM>(m.v0); t.v1 = rv_dpp_u32<CTRL, RM>(m.v1);    \
        const MinSt2 c = ms2_combine(t, m);                                                                           \
        if (TAKE) m = c;                                                                                              \
    }
    RV_WAVE_SCAN_STEPS(LF_STEP_)
#undef LF_STEP_
    return m;
}


// a sub-index as its wavefront sees it: the copy that holds it (cs / cl / cb, ranks [S, E)), and the same ranks of the other copy and of act[],
// which nothing uses until the split writes the children there -- scratch of the pick stage
struct LeafSub {
    const sa_t *cs; const u32 *cl; const uint8_t *cb;
    sa_t *ns; u32 *nl; uint16_t *act;
    int S, E, lane;
    Frame f;
    int64_t ra0, rb0;          // where the root's intervals begin (job-local positions: p - ra0, p - rb0)
    bool both;
    u32 minl; sa_t nsep0;
};

template <class PICK, class PARGS>
__device__ __forceinline__ void leaf_run(const RvLeafArgs &A, const PARGS &P) {
    // two copies of the arrays: a split reads one and writes the children into the other, a sub-index remembers which one holds it
    __shared__ sa_t  sa2[2][LN];
    __shared__ u32   lc2[2][LN];
    __shared__ uint8_t bw2[2][LN];
    __shared__ uint16_t act[LN];
    __shared__ Frame stack[MAXSTACK];
    __shared__ Frame cur[NW];
#ifdef RV_LEAF_PAD
    __shared__ u32 pad_[RV_LEAF_PAD / 4];      // (tuning: fewer workgroups per CU)
    if (A.minl == -12345) pad_[threadIdx.x] = 0;
#endif
    __shared__ int s_top, s_pending, s_lock;
    // The anchors of the root are collected here and leave with ONE reservation per workgroup: a reservation per anchor was
    // 1.7 x 10^6 returning atomics on one address per run of 2 x 250 Mbp, ~50 ns each at the L2 -- the launches took exactly that long.
    __shared__ u32 an_l[ACAP]; __shared__ sa_t an_a[ACAP], an_b[ACAP];
    __shared__ u32 s_na, s_base;
    __shared__ unsigned long long s_stats[4];

    const RvLeafRoot root = A.roots[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int i = tid; i < root.n; i += NT) {
        sa2[0][i] = A.SA[root.off + i]; lc2[0][i] = (u32)A.LCP[root.off + i]; bw2[0][i] = A.BWT[root.off + i] & RV_BWT_CHAR;      /* (the side bit is for the streaming scan; here SA is in LDS) */
    }
    if (tid == 0) {
        Frame f; f.start = 0; f.len = (int)root.n; f.depth = root.depth; f.buf = 0; f.a0 = root.a0; f.a1 = root.a1; f.b0 = root.b0; f.b1 = root.b1;
        cur[0] = f; s_top = 0; s_pending = 1; s_lock = 0; s_na = 0;
        s_stats[0] = s_stats[1] = s_stats[2] = s_stats[3] = 0;
    }
    __syncthreads();                                   // the only workgroup barrier
    const sa_t nsep0 = (sa_t)A.nsep0;
    const u32 minl = A.minl > 0 ? (u32)A.minl : 0u;
    const u32 acap = A.stage_cap < (u32)ACAP ? A.stage_cap : (u32)ACAP;
    u32 my_steps = 0, my_splits = 0, my_maxdepth = 0; u64 my_bp = 0;     // accumulated by lane 0 of every wave
    bool have = wv == 0;
#ifdef RV_LEAF_PROF
    long long pt = clock64(), p_idle = 0, p_scan = 0, p_split = 0, p_bub = 0;
#define LF_PROF(acc) { const long long now_ = clock64(); acc += now_ - pt; pt = now_; }
#else
#define LF_PROF(acc)
#endif

    for (;;) {
        LF_PROF(p_bub)
        if (!have) {
            // take a sub-index from the shared stack, or leave once every sub-index of the root is finished
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
        const Frame f = cur[wv];
        have = false;
        LF_PROF(p_idle)
        const int b = f.buf;
        sa_t *cs = sa2[b], *ns = sa2[b ^ 1];
        u32 *cl = lc2[b], *nl_ = lc2[b ^ 1];
        uint8_t *cb = bw2[b], *nb = bw2[b ^ 1];
        const int S = f.start, E = f.start + f.len;
        const bool both = f.a0 < f.a1 && f.b0 < f.b1;           // nsamples == 2 (reveal.c:1034-1041)
        if (lane == 0) { my_steps++; if ((u32)f.depth > my_maxdepth) my_maxdepth = (u32)f.depth; }

        u32 L = 0; int64_t pa = 0, pb = 0;
        LeafSub X; X.cs = cs; X.cl = cl; X.cb = cb; X.ns = ns; X.nl = nl_; X.act = act; X.S = S; X.E = E; X.lane = lane; X.f = f; X.both = both; X.minl = minl; X.nsep0 = nsep0; X.ra0 = root.a0; X.rb0 = root.b0;
        const bool picked = PICK::pick(A, P, X, L, pa, pb);
        LF_PROF(p_scan)
        if (!picked) {
            if (lane == 0) atomicSub(&s_pending, 1);
            continue;
        }
        if (lane == 0) {
            my_splits++; my_bp += L;
            const u32 k = atomicAdd(&s_na, 1u);
            if (k < acap) { an_l[k] = L; an_a[k] = (sa_t)pa; an_b[k] = (sa_t)pb; }
            else {                                   // (more anchors than the staging holds: minl of a few bases)
                const u32 slot = atomicAdd(A.anchor_count, 1u);
                if (slot < A.anchor_cap) { A.anchor_l[slot] = L; A.anchor_pos[2 * (size_t)slot] = pa; A.anchor_pos[2 * (size_t)slot + 1] = pb; }
            }
        }
        // (the matched text is lower-cased from the anchor list when the run ends: k_leaf_lower; nothing reads it before)
        // ---- linear graphalign: lead = left remainders, trail = right remainders ------------------
        const int64_t la0 = f.a0, la1 = pa, lb0 = f.b0, lb1 = pb;                     // leading intervals (may be empty)
        const int64_t ta0 = pa + L, ta1 = f.a1, tb0 = pb + L, tb1 = f.b1;             // trailing intervals
        // ---- label + split (reveal.c:1005-1117, 582-664) into the other copy: lead at S, trail right behind it ------
        // A sub-index holds exactly the suffixes of its intervals: the children's sizes follow from the interval lengths.  A lane
        // takes four consecutive ranks, so the wave-wide scans (counts, running minima) run once per 256 ranks.
        const usa_t LA0 = (usa_t)la0, LAn = la1 > la0 ? (usa_t)(la1 - la0) : 0, LB0 = (usa_t)lb0, LBn = lb1 > lb0 ? (usa_t)(lb1 - lb0) : 0;
        const usa_t TA0 = (usa_t)ta0, TAn = ta1 > ta0 ? (usa_t)(ta1 - ta0) : 0, TB0 = (usa_t)tb0, TBn = tb1 > tb0 ? (usa_t)(tb1 - tb0) : 0;
        const u32 nlead = (u32)(LAn + LBn);
        u32 cnt0 = 0, cnt1 = 0;                       // ranks already written to lead / trail
        MinSt2 car; car.has = 0; car.v0 = INF; car.v1 = INF;      // running-minimum carry
        for (int base = S; base < E; base += 4 * 64) {
            const int i0 = base + 4 * lane;
            u32 ev[4]; sa_t pos[4]; uint8_t bo[4]; u32 cls = 0;      // cls: two bits per rank (1 = lead, 2 = trail)
            MinSt2 agg; agg.has = 0; agg.v0 = INF; agg.v1 = INF;
            u32 n01 = 0;                                             // lead count | trail count << 16
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int i = i0 + r;
                u32 c = 0; ev[r] = INF; pos[r] = 0; bo[r] = 0;
                if (i < E) {
                    pos[r] = cs[i]; bo[r] = cb[i];
                    const usa_t p = (usa_t)pos[r];
                    if ((usa_t)(p - LA0) < LAn || (usa_t)(p - LB0) < LBn) c = 1;
                    else if ((usa_t)(p - TA0) < TAn || (usa_t)(p - TB0) < TBn) c = 2;
                    ev[r] = (i > S) ? cl[i] : INF;      // every rank of a leaf sub-index is labelled (lead, trail or matched): no skipped updates
                    if (c == 2 && (p == TA0 || p == TB0) && bo[r] >= 'A' && bo[r] <= 'Z') bo[r] += 32;   // its left neighbour was just matched
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
                    ns[S + e0] = pos[r]; nl_[S + e0] = e0 == 0 ? 0u : v; nb[S + e0] = bo[r];
                    e0++;
                } else if (c == 2) {
                    const u32 v = r1 < ev[r] ? r1 : ev[r];
                    ns[S + nlead + e1] = pos[r]; nl_[S + nlead + e1] = e1 == 0 ? 0u : v; nb[S + nlead + e1] = bo[r];
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
        LF_PROF(p_split)
        const int nl = (int)cnt0, ntr = (int)cnt1;
        if (lane == 0 && (cnt0 != nlead || cnt1 != (u32)(TAn + TBn))) PICK::fail(A, P, 8u);      // (a sub-index that is not the suffixes of its intervals)
        const int cdepth = f.depth + 1;
        bool do_lead = nl > 0, do_trail = ntr > 0;
        if (!A.trace) {
            // A child without both samples has nothing to match, and neither has one with an interval shorter than minl (bubble_sort
            // keeps every LCP value inside the intervals): counted as visited (reveal.c:1034-1041 / an empty scan), not scanned
            const int64_t need = minl > 1 ? (int64_t)minl : 1;
            if (do_lead && !(la1 - la0 >= need && lb1 - lb0 >= need)) { do_lead = false; if (lane == 0) { my_steps++; if ((u32)cdepth > my_maxdepth) my_maxdepth = (u32)cdepth; } }
            if (do_trail && !(ta1 - ta0 >= need && tb1 - tb0 >= need)) { do_trail = false; if (lane == 0) { my_steps++; if ((u32)cdepth > my_maxdepth) my_maxdepth = (u32)cdepth; } }
        }
        // ---- bubble_sort on the leading child, cuts in ascending order (reveal.c:666-727); a child nobody scans needs none ----
        for (int cut = 0; cut < 2 && do_lead; cut++) {
            const int64_t B = cut == 0 ? pa : pb;
            const int64_t ib = cut == 0 ? la0 : lb0;
            if (!(ib < B)) continue;                                        // no leading interval ends at this cut
            const int64_t wlo = (B - (int64_t)A.lcap > ib) ? B - (int64_t)A.lcap : ib;
            // actives in rank order
            u32 nact = 0;
            for (int base = 0; base < nl; base += 64) {
                const int e = base + lane;
                bool on = false;
                if (e < nl) {
                    const int64_t p = (int64_t)ns[S + e];
                    if (p >= wlo && p < B) {
                        const int64_t l0 = (int64_t)nl_[S + e], l1 = (e + 1 < nl) ? (int64_t)nl_[S + e + 1] : 0;
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
                const int64_t p = (int64_t)ns[S + e], l0 = (int64_t)nl_[S + e];          // (the same address for every lane: one broadcast read)
                if (p < B && p + l0 > B) {
                    const int64_t t = B - p; const uint8_t tB = nb[S + e];
                    // x = largest r <= e with r == 0 or LCP[r] < t
                    int x = 0;
                    for (int hi = e;; hi -= 64) {
                        const int r = hi - lane;
                        const u64 mask = __ballot(r >= 0 && (r == 0 || (int64_t)nl_[S + r] < t));
                        if (mask) { x = hi - (int)__builtin_ctzll(mask); break; }
                    }
                    const u32 lnext = (e < nl - 1) ? nl_[S + e + 1] : 0u;
                    // shift [x, e-1] -> [x+1, e], from the top in pieces of 64: a piece reads below what it writes, the wave reads before it writes
                    for (int hi = e; hi > x; hi -= 64) {
                        const int r = hi - lane;
                        sa_t vs = 0; u32 vl = 0; uint8_t vb = 0;
                        if (r > x) { vs = ns[S + r - 1]; vl = nl_[S + r - 1]; vb = nb[S + r - 1]; }
                        RV_WSYNC();
                        if (r > x) { ns[S + r] = vs; nl_[S + r] = vl; nb[S + r] = vb; }
                        RV_WSYNC();
                    }
                    if (lane == 0) {
                        ns[S + x] = (sa_t)p; nb[S + x] = tB;
                        if (x + 1 < nl) nl_[S + x + 1] = (u32)t;
                        if (e < nl - 1 && l0 < (int64_t)lnext) nl_[S + e + 1] = (u32)l0;
                    }
                } else if (e < nl - 1) {
                    const int64_t l1 = (int64_t)nl_[S + e + 1];
                    if (lane == 0 && p < B && p + l1 > B && l1 > l0) nl_[S + e + 1] = (u32)(B - p);
                }
                RV_WSYNC();
            }
        }
        // ---- children (reveal.c:1296-1324); their order is free: this wave goes on with the smaller one, the larger one goes to
        // the stack for any wave (the stack stays O(waves x log n) deep whatever the shape of the tree) -------------------------
        if (lane == 0) {
            const bool keep_lead = do_lead && (!do_trail || nl <= ntr);      // which child this wave goes on with (if any)
            if (do_lead && do_trail) {
                while (atomicCAS(&s_lock, 0, 1) != 0) __builtin_amdgcn_s_sleep(1);
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                const int t = s_top;
                if (t < MAXSTACK) {
                    Frame *o = &stack[t];                                     // the other child
                    o->start = keep_lead ? S + nl : S; o->len = keep_lead ? ntr : nl; o->depth = cdepth; o->buf = b ^ 1;
                    o->a0 = keep_lead ? ta0 : la0; o->a1 = keep_lead ? ta1 : la1; o->b0 = keep_lead ? tb0 : lb0; o->b1 = keep_lead ? tb1 : lb1;
                    s_top = t + 1; atomicAdd(&s_pending, 1);
                } else PICK::fail(A, P, 4u);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                atomicExch(&s_lock, 0);
            }
            if (do_lead || do_trail) {
                Frame *o = &cur[wv];
                o->start = keep_lead ? S : S + nl; o->len = keep_lead ? nl : ntr; o->depth = cdepth; o->buf = b ^ 1;
                o->a0 = keep_lead ? la0 : ta0; o->a1 = keep_lead ? la1 : ta1; o->b0 = keep_lead ? lb0 : tb0; o->b1 = keep_lead ? lb1 : tb1;
            } else {
                atomicSub(&s_pending, 1);
            }
        }
        have = do_lead || do_trail;
    }
    if (lane == 0) {
        atomicAdd(&s_stats[0], (unsigned long long)my_steps); atomicAdd(&s_stats[1], (unsigned long long)my_splits);
        atomicAdd(&s_stats[2], (unsigned long long)my_bp); atomicMax(&s_stats[3], (unsigned long long)my_maxdepth);
#ifdef RV_LEAF_PROF
        atomicAdd(&A.stats[4], (unsigned long long)p_idle); atomicAdd(&A.stats[5], (unsigned long long)p_scan);
        atomicAdd(&A.stats[6], (unsigned long long)p_split); atomicAdd(&A.stats[7], (unsigned long long)p_bub);
#endif
    }
    __syncthreads();                                   // every wave has left the loop: the root is finished
    const u32 na = s_na < acap ? s_na : acap;
    if (tid == 0) {
        s_base = na ? atomicAdd(A.anchor_count, na) : 0u;
        atomicAdd(&A.stats[0], s_stats[0]); atomicAdd(&A.stats[1], s_stats[1]); atomicAdd(&A.stats[2], s_stats[2]); atomicMax(&A.stats[3], s_stats[3]);
    }
    __syncthreads();
    for (u32 k = tid; k < na; k += NT) {
        const size_t slot = (size_t)s_base + k;
        if (slot < A.anchor_cap) { A.anchor_l[slot] = an_l[k]; A.anchor_pos[2 * slot] = (int64_t)an_a[k]; A.anchor_pos[2 * slot + 1] = (int64_t)an_b[k]; }
    }
}

}  // namespace
