// rv_leaf.hip -- the tail of the recursion inside one workgroup.
//
// The recursion of aligner() (reveallib/reveal.c:731-1338) produces ~10^5
// sub-indices per 10 Mbp, most of a few hundred ranks.  Once a sub-index of a
// two-sample alignment has at most RV_LEAF_N ranks, its whole sub-tree is
// finished here by one workgroup with the arrays in LDS -- one wavefront per sub-index, the waves of the workgroup taking
// sub-indices of the root's tree from a shared stack, no workgroup barrier in between:
//   scan   getmums_rem predicate                      reveal.c:119-180
//   pick   built-in picker (longest full match, ties -> smallest coordinate)
//   split  D-label + stable partition + running-min LCP + lower-casing   reveal.c:1005-1234, 582-664
//   bubble bubble_sort on the leading child, cuts in ascending order     reveal.c:666-727
// Same arithmetic as the level kernels (rv_scan.hip, rv_split.hip), so every
// sub-index has the same SA/LCP as in the reference; only used with the built-in
// callbacks (rv_align_builtin), never when Python callbacks drive the recursion.
// The body is leaf_run (rv_leaf_stages.h), instantiated here with the built-in picker as its pick stage and in rv_leaf_chain.hip with the
// reference's default picker (k_leaf_chain, rv_many's pair jobs under rv_many_set_picker).
#include "rv_leaf_stages.h"

namespace {

struct NoArgs {};
// the built-in picker: the longest match present in both samples, ties -> the smallest coordinate
struct PickBuiltin {
    static __device__ __forceinline__ void fail(const RvLeafArgs &A, const NoArgs &, u32 bits) { atomicOr(A.err, bits); }
    static __device__ __forceinline__ bool pick(const RvLeafArgs &A, const NoArgs &, const LeafSub &X, u32 &L, int64_t &pa, int64_t &pb) {
        const sa_t *cs = X.cs; const u32 *cl = X.cl; const uint8_t *cb = X.cb;
        const int S = X.S, E = X.E, lane = X.lane;
        const Frame &f = X.f;
        const bool both = X.both; const u32 minl = X.minl; const sa_t nsep0 = X.nsep0;
        // ---- scan (reveal.c:131-159) + picker ------------------------------------------------
        u64 best = 0; sa_t bpart = 0;          // the lane's best candidate and its other member
        u64 hsa = 0, hlc = 0;
        for (int i = S + lane; i < E; i += 64) {
            if (A.trace) { hsa = hash_step(hsa, (u64)(i - S), (int64_t)cs[i]); hlc = hash_step(hlc, (u64)(i - S), (int64_t)cl[i]); }
            if (i == S) continue;
            const u32 l = cl[i];
            if (l < minl) continue;
            const sa_t s1 = cs[i], s0 = cs[i - 1];
            if ((s1 > nsep0) == (s0 > nsep0)) continue;
            const u32 la = (i + 1 < E) ? cl[i + 1] : 0u;
            if (!(cl[i - 1] < l && la < l)) continue;
            const bool ok = s1 < s0 ? left_maximal(cb[i], cb[i - 1]) : left_maximal(cb[i - 1], cb[i]);
            if (!ok) continue;
            const u64 a = (u64)(s1 < s0 ? s1 : s0);
            const u64 key = ((u64)l << 40) | (0xFFFFFFFFFFull - a);           // longest, then smallest position (< 2^40)
            if (key > best) { best = key; bpart = s1 < s0 ? s0 : s1; }
        }
        u64 hm = 0; u32 total_cand = 0;
        if (A.trace) {
            // scan-result hash needs each candidate's ordinal in rank order: second pass with a running count
            u32 run = 0;
            for (int base = S; base < E; base += 64) {
                const int i = base + lane;
                bool ok = false; u32 l = 0; sa_t s1 = 0, s0 = 0;
                if (i < E && i > S) {
                    l = cl[i]; s1 = cs[i]; s0 = cs[i - 1];
                    const u32 la = (i + 1 < E) ? cl[i + 1] : 0u;
                    ok = l >= minl && ((s1 > nsep0) != (s0 > nsep0)) && cl[i - 1] < l && la < l &&
                         (s1 < s0 ? left_maximal(cb[i], cb[i - 1]) : left_maximal(cb[i - 1], cb[i]));
                }
                const u64 mask = __ballot(ok);
                const u32 k = run + rv_lanes_below(mask);
                if (ok) {
                    const int64_t a = (int64_t)(s1 < s0 ? s1 : s0), bb = (int64_t)(s1 < s0 ? s0 : s1);
                    const u64 o = (u64)k * 6;                  // the candidate as the oracle hashes it: l, n = 2, (0, a), (1, b)
                    hm = hash_step(hm, o, (int64_t)l); hm = hash_step(hm, o + 1, 2); hm = hash_step(hm, o + 2, 0);
                    hm = hash_step(hm, o + 3, a); hm = hash_step(hm, o + 4, 1); hm = hash_step(hm, o + 5, bb);
                }
                run += (u32)__popcll(mask);
            }
            total_cand = run;
            hsa = wave_sum_u64(hsa); hlc = wave_sum_u64(hlc); hm = wave_sum_u64(hm);
        }
        const u64 mine = best;
        best = wave_max_u64(best);
        const bool picked = both && best != 0;
        L = (u32)(best >> 40);
        pa = (int64_t)(0xFFFFFFFFFFull - (best & 0xFFFFFFFFFFull));
        pb = 0;
        if (picked) {
            // the other member of the chosen match: held by the one lane whose candidate won (a position pairs with one rank only)
            const int owner = (int)__builtin_ctzll(__ballot(mine == best));
            const u64 bp = (u64)bpart;
            pb = (int64_t)(((u64)(u32)__builtin_amdgcn_readlane((int)(u32)(bp >> 32), owner) << 32) | (u32)__builtin_amdgcn_readlane((int)(u32)bp, owner));
        }
        if (A.trace && lane == 0) {
            const u32 slot = atomicAdd(A.trace_count, 1u);
            if (slot < A.trace_cap) {
                rv_trace t;
                t.key = f.a0 < f.a1 ? f.a0 : f.b0; t.n = f.len; t.depth = f.depth; t.nsamples = (f.a0 < f.a1) + (f.b0 < f.b1);
                t.nnodes = t.nsamples; t.picked = picked ? 1 : 0; t.nmums = total_cand; t.l = picked ? L : 0; t.mn = picked ? 2 : 0;
                t.sp_min = picked ? pa : 0; t.h_sa = hsa; t.h_lcp = hlc; t.h_mums = hm;
                A.trace_out[slot] = t;
            }
        }
        return picked;
    }
};

__global__ __launch_bounds__(NT) void k_leaf(RvLeafArgs A) { leaf_run<PickBuiltin>(A, NoArgs()); }

// the matched text of the anchors the leaf launches found, lower-cased when the run ends (reveal.c:1230-1234): four anchors per wave -- sixteen lanes
// per anchor, eight per side, sixteen bytes per lane and step.  (One wave per anchor, half a wave per side and eight bytes per lane: 2 x 10^6 waves of
// three dependent trips to memory each -- length, positions, text -- were 1.2 ms at 2 x 250 Mbp for 1 GB of traffic; a byte per lane 1.07 ms for
// 2 x 10^6 anchors of ~120 bases.)  The anchors of a run cover disjoint text, and whole 16-byte pieces never reach beyond the match.
__device__ inline u64 lower8(u64 x) {
    // 0x20 in every byte of 'A' .. 'Z': bit 7 of (b + 0x3F) is set from 'A' on, bit 7 of (b + 0x25) from '[' on (bytes below 0x80)
    const u64 lo7 = x & 0x7F7F7F7F7F7F7F7Full;
    return x | (((lo7 + 0x3F3F3F3F3F3F3F3Full) & ~(lo7 + 0x2525252525252525ull) & ~x & 0x8080808080808080ull) >> 2);
}
// An anchor longer than LOWER_CAP bytes (near-identical inputs: one anchor of 50 Mbp took its eight lanes 183 ms) is only begun here: it goes
// to a short list, and k_leaf_lower_long shares what is left of it among a whole grid.  (A full list: the anchor is finished here after all.)
constexpr int64_t LOWER_CAP = 16384;
constexpr u32 LOWER_LONG_MAX = 4096;
__global__ __launch_bounds__(NT) void k_leaf_lower(uint8_t *__restrict__ T, const int64_t *__restrict__ pos, const u32 *__restrict__ len, u32 na, u32 *__restrict__ lng) {
    const int64_t t = (int64_t)blockIdx.x * NT + threadIdx.x;
    const u32 e = (u32)(t >> 4);
    if (e >= na) return;
    int64_t l = (int64_t)len[e];
    const int side = (int)(t >> 3) & 1, h = (int)t & 7;
    if (l > LOWER_CAP) {      // (both sides and all eight lanes see the same slot: the first lane of the first side takes it, the others learn it through the wave)
        u32 slot = 0;
        if (side == 0 && h == 0) slot = atomicAdd(&lng[0], 1u);
        slot = (u32)__shfl((int)slot, (int)(threadIdx.x & 63) & ~15, 64);
        if (slot < LOWER_LONG_MAX) {
            if (side == 0 && h == 0) lng[4 + slot] = e;
            l = LOWER_CAP;      // (a multiple of sixteen: the tail loop below does nothing)
        }
    }
    uint8_t *const p = T + pos[2 * (size_t)e + side];
    for (int64_t j = (int64_t)h * 16; j + 16 <= l; j += 128) {
        u64 x[2];
        __builtin_memcpy(x, p + j, 16);
        x[0] = lower8(x[0]); x[1] = lower8(x[1]);
        __builtin_memcpy(p + j, x, 16);
    }
    for (int64_t j = (l & ~(int64_t)15) + h; j < l; j += 8) { const uint8_t ch = p[j]; if (ch >= 'A' && ch <= 'Z') p[j] = ch + 32; }
}
// the rest of the long anchors: every workgroup takes 4 KB pieces of every listed anchor in turn (both sides), sixteen bytes per lane and step
__global__ __launch_bounds__(NT) void k_leaf_lower_long(uint8_t *__restrict__ T, const int64_t *__restrict__ pos, const u32 *__restrict__ len, const u32 *__restrict__ lng) {
    const u32 cnt = lng[0] < LOWER_LONG_MAX ? lng[0] : LOWER_LONG_MAX;
    for (u32 k = 0; k < cnt; k++) {
        const u32 e = lng[4 + k];
        const int64_t l = (int64_t)len[e];
        for (int side = 0; side < 2; side++) {
            uint8_t *const p = T + pos[2 * (size_t)e + side];
            for (int64_t j0 = LOWER_CAP + (int64_t)blockIdx.x * (NT * 16); j0 < l; j0 += (int64_t)gridDim.x * (NT * 16)) {
                const int64_t j = j0 + (int64_t)threadIdx.x * 16;
                if (j + 16 <= l) {
                    u64 x[2];
                    __builtin_memcpy(x, p + j, 16);
                    x[0] = lower8(x[0]); x[1] = lower8(x[1]);
                    __builtin_memcpy(p + j, x, 16);
                } else {
                    for (int64_t i = j; i < l; i++) { const uint8_t ch = p[i]; if (ch >= 'A' && ch <= 'Z') p[i] = ch + 32; }
                }
            }
        }
    }
}

}  // namespace

int rv_leaf_launch(Workspace &ws, const RvLeafArgs &a, int nroots) {
    if (nroots <= 0) return 0;
    hipLaunchKernelGGL(k_leaf, dim3((unsigned)nroots), dim3(NT), 0, ws.stream, a);
    RV_LAUNCH_CHECK();
    return 0;
}

int rv_leaf_lower_launch(Workspace &ws, uint8_t *T, const int64_t *pos, const u32 *len, u32 na) {
    if (na == 0) return 0;
    RV_TRY(ws.misc[15].reserve((size_t)(4 + LOWER_LONG_MAX) * 4));
    u32 *lng = ws.misc[15].as<u32>();
    RV_HIP(hipMemsetAsync(lng, 0, 16, ws.stream));
    hipLaunchKernelGGL(k_leaf_lower, dim3((unsigned)ceil_div((int64_t)na * 16, NT)), dim3(NT), 0, ws.stream, T, pos, len, na, lng);
    RV_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_leaf_lower_long, dim3(1024), dim3(NT), 0, ws.stream, T, pos, len, (const u32 *)lng);
    RV_LAUNCH_CHECK();
    return 0;
}
