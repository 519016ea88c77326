// rv_glocal.hip -- the glocal chain of `reveal transform` (transform.py:301-360, 947-1180; useheap=False) on a block list.
//
// The rule is stated in include/reveal_amd.h (rv_glocal_filter).  A pass on an axis: the list plus a dummy per sequence end of that axis, stably
// sorted by (position, -score); H[0] = `start`, H[k] = the k-th entry in sorted order.  The window of H[k] -- which predecessors the reference's
// walk back looks at -- depends on coordinates only, and so do the two filters and every cost; what is left of the loop is
//     score[k] = max over the window (score[p] - c(p, k)) + alfa * score of the block,   ties to the nearest p.
//
// Device programme of a pass: k_glc_keys -> rv_radix_sort_pairs (one 64-bit key (position, inverted score) where both fit, two stable sorts
// otherwise) -> k_glc_gather (the entries in sorted order, in the axis' coordinates) -> rv_inclusive_max_u64 of the ends -> k_glc_window (a
// thread per block: binary search for `deepest`, the walk back that counts unfiltered predecessors) -> rv_exclusive_sum_u64 of the window lengths
// -> per tile of at most RV_GLOCAL_EDGE_BUDGET edges: k_glc_cost (a thread per edge: filter and cost, 8 bytes) and k_glc_chain (ONE wavefront:
// the recurrence, 64 edges a step) in stream order -> k_glc_double x ceil(log2 n) (the path from `end` marked by pointer doubling; no thread walks
// the back-pointers) -> rv_exclusive_sum_u32 -> k_glc_compact (the real blocks on the path, in sorted order: the next pass' list).  Per pass the
// host reads the edge total, the longest window and `end` (they size the tiles) and the survivors' count; the chain comes back once, as indices.
#include "rv_glocal.h"
#include <algorithm>
#include <numeric>

namespace {

// a block list in device memory: five int64 arrays of cap, then four int32 arrays of cap (idx = the block's number in the caller's list)
struct GlcList {
    int64_t *s1, *e1, *s2, *e2, *score; int32_t *o, *refid, *ctgid, *idx;
    __host__ __device__ GlcList() {}
    __host__ __device__ GlcList(void *p, size_t cap) {
        s1 = (int64_t *)p; e1 = s1 + cap; s2 = e1 + cap; e2 = s2 + cap; score = e2 + cap;
        o = (int32_t *)(score + cap); refid = o + cap; ctgid = refid + cap; idx = ctgid + cap;
    }
};
constexpr size_t GLC_LIST_BYTES = 5 * 8 + 4 * 4;

// the entries of a pass in sorted order, index 0 = `start`: m + 2 slots each
struct GlcH {
    int64_t *a, *ae, *b, *be, *sc; int32_t *o, *id1, *id2;
    __device__ __forceinline__ GlcEntry at(u32 k) const { GlcEntry e; e.a = a[k]; e.ae = ae[k]; e.b = b[k]; e.be = be[k]; e.o = o[k]; e.id1 = id1[k]; e.id2 = id2[k]; return e; }
};

struct GlcPass {
    GlcList L; u32 n, nd, m;      // the list, its length, the dummies of this axis, m = n + nd
    const int64_t *dpos;         // their positions
    int64_t startpos;
    int axis;
};

__device__ __forceinline__ int64_t glc_pos(const GlcPass &P, u32 i) { return i < P.n ? (P.axis ? P.L.s2[i] : P.L.s1[i]) : P.dpos[i - P.n]; }

// mode 0: (position << sbits) | inverted score;  mode 1: inverted score (the first of two stable sorts);  mode 2: position of the entry at sorted
// position i of the first sort
__global__ __launch_bounds__(256) void k_glc_keys(GlcPass P, int mode, int sbits, int64_t maxscore, const u32 *__restrict__ perm, u64 *__restrict__ keys, u32 *__restrict__ vals) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= P.m) return;
    if (mode == 2) { const u32 r = perm[i]; keys[i] = (u64)glc_pos(P, r); vals[i] = r; return; }
    const u64 inv = (u64)(maxscore - (i < P.n ? P.L.score[i] : 0));
    keys[i] = mode == 0 ? (((u64)glc_pos(P, i) << sbits) | inv) : inv;
    vals[i] = i;
}

// hdr: [0] the sorted position of `end`, [1] the longest window, [2] survivors
__global__ __launch_bounds__(256) void k_glc_gather(GlcPass P, const u32 *__restrict__ perm, GlcH H, u64 *__restrict__ ends, int64_t *__restrict__ score, u32 *__restrict__ back, u32 *__restrict__ hdr) {
    const u32 k = blockIdx.x * 256u + threadIdx.x;
    if (k > P.m) return;
    if (k == 0) {
        H.a[0] = H.ae[0] = P.startpos; H.b[0] = H.be[0] = 0; H.sc[0] = 0; H.o[0] = 0; H.id1[0] = -1; H.id2[0] = -1;
        ends[0] = 0; score[0] = 0; back[0] = 0;
        return;
    }
    const u32 r = perm[k - 1];
    if (r < P.n) {
        const GlcList &L = P.L;
        const bool ax = P.axis != 0;
        H.a[k] = ax ? L.s2[r] : L.s1[r]; H.ae[k] = ax ? L.e2[r] : L.e1[r]; H.b[k] = ax ? L.s1[r] : L.s2[r]; H.be[k] = ax ? L.e1[r] : L.e2[r];
        H.sc[k] = L.score[r]; H.o[k] = L.o[r]; H.id1[k] = ax ? L.ctgid[r] : L.refid[r]; H.id2[k] = ax ? L.refid[r] : L.ctgid[r];
    } else {
        const int64_t pos = P.dpos[r - P.n];
        H.a[k] = H.ae[k] = pos; H.b[k] = H.be[k] = 0; H.sc[k] = 0; H.o[k] = 0; H.id1[k] = -1; H.id2[k] = -1;
        if (r == P.m - 1) hdr[0] = k;
    }
    ends[k] = (u64)H.ae[k];
}

// wlen[k] = how many entries H[k]'s walk back covers, H[k-1] down to its far end; wlen[0] = wlen[m+1] = 0
__global__ __launch_bounds__(256) void k_glc_window(GlcH H, const u64 *__restrict__ rmax, u32 m, int64_t lastn, int64_t lastbp, u64 *__restrict__ wlen, u32 *__restrict__ hdr) {
    const u32 k = blockIdx.x * 256u + threadIdx.x;
    u32 w = 0;
    if (k >= 1 && k <= m) {
        const int64_t ba = H.a[k], bae = H.ae[k], bb = H.b[k], bbe = H.be[k]; const int32_t bid = H.id1[k];
        u32 lo = 1, hi = k;                                                  // deepest: the first entry whose end reaches ba (H[k] itself does)
        while (lo < hi) { const u32 mid = lo + ((hi - lo) >> 1); if (rmax[mid] >= (u64)ba) hi = mid; else lo = mid + 1; }
        const int64_t da = H.a[lo];
        int64_t l = 0;
        u32 far = 0;
        for (u32 p = k - 1; p > 0; p--) {
            const int64_t pa = H.a[p];
            if (glc_skip(pa, H.ae[p], H.b[p], H.be[p], H.id1[p], ba, bae, bb, bbe, bid)) continue;
            l++;
            if (ba - pa > lastbp && l >= lastn && pa < da) { far = p; break; }
        }
        w = k - far;
    }
    if (k <= m + 1) wlen[k] = w;
    const u32 wm = (u32)rv_wave_max_u64((u64)w);
    if ((threadIdx.x & 63) == 0 && wm) atomicMax(&hdr[1], wm);
}

// the blocks of tile t: those whose first edge lies in [t * budget, (t + 1) * budget) -> [klo, khi)
__device__ __forceinline__ u32 glc_first_at(const u64 *__restrict__ eoff, u32 m, u64 x) {      // the first k in [1, m + 1] with eoff[k] >= x
    u32 lo = 1, hi = m + 1;
    while (lo < hi) { const u32 mid = lo + ((hi - lo) >> 1); if (eoff[mid] >= x) hi = mid; else lo = mid + 1; }
    return lo;
}

// E[j] of the tile: the cost of edge j (block k, predecessor k - 1 - its number inside the block: nearest first), -1 where a filter drops it
__global__ __launch_bounds__(256) void k_glc_cost(GlcH H, const u64 *__restrict__ eoff, u32 m, u64 tile, u64 budget, int axis, RvGlcParams w, const int64_t *__restrict__ rs,
                                                   const int64_t *__restrict__ re, int64_t *__restrict__ E, u64 ecap) {
    __shared__ u32 s_k[2];
    if (threadIdx.x < 2) s_k[threadIdx.x] = glc_first_at(eoff, m, (tile + threadIdx.x) * budget);
    __syncthreads();
    const u32 klo = s_k[0], khi = s_k[1];
    if (klo >= khi) return;
    const u64 base = eoff[klo], j = (u64)blockIdx.x * 256u + threadIdx.x, g = base + j;
    if (g >= eoff[khi] || j >= ecap) return;
    u32 lo = klo, hi = khi;                                                  // the last k in [klo, khi) with eoff[k] <= g
    while (hi - lo > 1) { const u32 mid = lo + ((hi - lo) >> 1); if (eoff[mid] <= g) lo = mid; else hi = mid; }
    const u32 k = lo, p = k - 1 - (u32)(g - eoff[k]);
    const GlcEntry b = H.at(k), q = H.at(p);
    E[j] = glc_skip(q.a, q.ae, q.b, q.be, q.id1, b.a, b.ae, b.b, b.be, b.id1) ? (int64_t)-1 : glc_cost(q, b, axis, w, rs, re);
}

// The recurrence over the blocks of a tile: ONE wavefront, a block's edges 64 at a time.  Nothing but score[] depends on the step before, so the
// wavefront works in groups of GLC_G blocks: the first GLC_NR * 64 costs of every block of the NEXT group are loaded before this group is worked
// through, and the window bounds and gains of the group after that (a lane per block, handed round by readlane) -- a step then waits for LDS and
// for its own reduction, not for memory.  Inside the wavefront the order of its own LDS and global accesses is the hardware's; the fence per step
// is of wavefront scope and costs no wait.  Scores of the last GLC_RING entries sit in LDS; older ones are read from global memory (this
// wavefront or an earlier launch wrote them).
constexpr u32 GLC_RING = 2048;
constexpr int GLC_G = 8, GLC_NR = 3;
static_assert((u32)GLC_NR * 64 <= GLC_RING, "the rounds loaded ahead read their scores from the ring");
constexpr u64 GLC_SIGN = 0x8000000000000000ull;
__device__ __forceinline__ u64 glc_lane64(u64 v, int i) {
    return ((u64)(u32)__builtin_amdgcn_readlane((int)(u32)(v >> 32), i) << 32) | (u32)__builtin_amdgcn_readlane((int)(u32)v, i);
}
// maximum of a u32 over the wavefront, in every lane: the DPP moves fold into the v_max_u32 they feed (as rv_wave_min_u32's do), six VALU
// instructions and a readlane -- a 64-bit maximum by shifted copies costs a 64-bit compare and two selects at each of its six steps
__device__ __forceinline__ u32 glc_wave_max_u32(u32 v) {
    int x = (int)v, y;
#define GLC_DPP_MAX(ctrl, rmask)                                                       \
    y = __builtin_amdgcn_update_dpp(0, x, ctrl, rmask, 0xf, false);                    \
    x = (int)(((u32)y > (u32)x) ? (u32)y : (u32)x);
    GLC_DPP_MAX(0xB1, 0xf)     // quad_perm [1,0,3,2]
    GLC_DPP_MAX(0x4E, 0xf)     // quad_perm [2,3,0,1]
    GLC_DPP_MAX(0x141, 0xf)    // row_half_mirror
    GLC_DPP_MAX(0x140, 0xf)    // row_mirror: every lane of a row holds the row's maximum
    GLC_DPP_MAX(0x142, 0xa)    // row_bcast:15 into rows 1 and 3
    GLC_DPP_MAX(0x143, 0xc)    // row_bcast:31 into rows 2 and 3: lane 63 holds the wave's maximum
#undef GLC_DPP_MAX
    return (u32)__builtin_amdgcn_readlane(x, 63);
}
#define GLC_WAVE_ORDER() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)
__global__ __launch_bounds__(64) void k_glc_chain(const u64 *__restrict__ eoff, const int64_t *__restrict__ sc, u32 m, u64 tile, u64 budget, int64_t alfa, const int64_t *__restrict__ E,
                                                   u64 ecap, int64_t *score, u32 *back) {
    __shared__ int64_t ring[GLC_RING];
    const u32 lane = threadIdx.x;
    const u32 klo = glc_first_at(eoff, m, tile * budget), khi = glc_first_at(eoff, m, (tile + 1) * budget);
    if (klo >= khi) return;
    for (u32 p = (klo > GLC_RING ? klo - GLC_RING : 0) + lane; p < klo; p += 64) ring[p & (GLC_RING - 1)] = score[p];
    RV_WSYNC();
    const u64 base = eoff[klo];
    // lane i of a group's meta words: eoff[kg + i] (lanes 0 .. GLC_G) and the score of block kg + i (nothing is computed from them before their
    // group's turn: a use is a wait)
    auto meta_e = [&](u32 kg) -> u64 { const u32 k = kg + lane; return (lane <= (u32)GLC_G && k <= khi) ? eoff[k] : 0ull; };
    auto meta_a = [&](u32 kg) -> int64_t { const u32 k = kg + lane; return (lane < (u32)GLC_G && k < khi) ? sc[k] : (int64_t)0; };
    auto fetch = [&](u64 me, u32 kg, int64_t (&c)[GLC_G][GLC_NR]) {
#pragma unroll
        for (int i = 0; i < GLC_G; i++) {
            const u64 e0 = glc_lane64(me, i), e1 = glc_lane64(me, i + 1);
            const u64 w = kg + (u32)i < khi ? e1 - e0 : 0;
#pragma unroll
            for (int r = 0; r < GLC_NR; r++) {
                const u64 j = (u64)r * 64 + lane;
                c[i][r] = (j < w && e0 - base + j < ecap) ? E[e0 - base + j] : (int64_t)-1;
            }
        }
    };
    u64 me0 = meta_e(klo), me1 = meta_e(klo + GLC_G);
    int64_t ma0 = meta_a(klo), ma1 = meta_a(klo + GLC_G);
    int64_t cc[GLC_G][GLC_NR], cn[GLC_G][GLC_NR];
    fetch(me0, klo, cc);
    for (u32 kg = klo; kg < khi; kg += GLC_G) {
        const u64 me2 = meta_e(kg + 2 * GLC_G);
        const int64_t ma2 = meta_a(kg + 2 * GLC_G);
        fetch(me1, kg + GLC_G, cn);
#pragma unroll
        for (int i = 0; i < GLC_G; i++) {
            const u32 k = kg + (u32)i;
            if (k >= khi) break;
            const u64 e0 = glc_lane64(me0, i), w = glc_lane64(me0, i + 1) - e0;
            const int64_t add = alfa * (int64_t)glc_lane64((u64)ma0, i);
            u64 bestv = 0; u32 bestj = 0;
            // the costs of edges r .. r + 63, -1 where there is none.  The rounds loaded ahead reach back less than GLC_RING entries: no access to
            // global memory stands in a step's way there (a load that might have happened is waited for, and with it this wavefront's own stores)
            auto round = [&](u64 r, int64_t c, bool near) {
                u64 v = 0;
                if (c >= 0) {
                    const u64 j = r + lane;
                    const u32 p = k - 1 - (u32)j;
                    const int64_t s = (near || j < GLC_RING) ? ring[p & (GLC_RING - 1)] : score[p];
                    v = (u64)(s - c) ^ GLC_SIGN;
                }
                // the 64-bit maximum as two 32-bit ones: the high words, then the low words of the lanes that hold the highest high word
                const u32 hi = (u32)(v >> 32), mh = glc_wave_max_u32(hi);
                const u32 lo = hi == mh ? (u32)v : 0u, ml = glc_wave_max_u32(lo);
                const u64 mx = ((u64)mh << 32) | ml;
                if (mx > bestv) {                                            // (an earlier round holds nearer predecessors: it keeps a tie)
                    bestv = mx;
                    bestj = (u32)r + (u32)__builtin_ctzll(__ballot(v == mx));
                }
            };
#pragma unroll
            for (int r = 0; r < GLC_NR; r++)
                if ((u64)r * 64 < w) round((u64)r * 64, cc[i][r], true);
            for (u64 r = (u64)GLC_NR * 64; r < w; r += 64) {
                const u64 j = r + lane;
                round(r, (j < w && e0 - base + j < ecap) ? E[e0 - base + j] : (int64_t)-1, false);
            }
            const int64_t s = (int64_t)(bestv ^ GLC_SIGN) + add;
            if (lane == 0) { score[k] = s; back[k] = k - 1 - bestj; ring[k & (GLC_RING - 1)] = s; }
            GLC_WAVE_ORDER();
        }
#pragma unroll
        for (int i = 0; i < GLC_G; i++)
#pragma unroll
            for (int r = 0; r < GLC_NR; r++) cc[i][r] = cn[i][r];
        me0 = me1; me1 = me2; ma0 = ma1; ma1 = ma2;
    }
}

// M <- M u J(M), J <- J o J
__global__ __launch_bounds__(256) void k_glc_mark_init(u32 m, const u32 *__restrict__ hdr, u32 *__restrict__ M) {
    const u32 k = blockIdx.x * 256u + threadIdx.x;
    if (k <= m + 1) M[k] = (k == hdr[0]) ? 1u : 0u;
}
__global__ __launch_bounds__(256) void k_glc_double(u32 m, const u32 *__restrict__ Jin, u32 *__restrict__ Jout, u32 *M) {
    const u32 k = blockIdx.x * 256u + threadIdx.x;
    if (k > m) return;
    const u32 j = Jin[k];
    if (M[k]) M[j] = 1u;      // (a mark set earlier in this launch only adds entries further down the same path)
    Jout[k] = Jin[j];
}
// keep[k] = 1 for a real block on the path, in place of the marks
__global__ __launch_bounds__(256) void k_glc_keep(u32 m, const int32_t *__restrict__ id1, u32 *M) {
    const u32 k = blockIdx.x * 256u + threadIdx.x;
    if (k > m + 1) return;
    M[k] = (k >= 1 && k <= m && M[k] && id1[k] >= 0) ? 1u : 0u;
}
__global__ __launch_bounds__(256) void k_glc_compact(GlcPass P, const u32 *__restrict__ perm, const u32 *__restrict__ koff, GlcList W, u32 *__restrict__ hdr) {
    const u32 k = blockIdx.x * 256u + threadIdx.x;
    if (k > P.m) return;
    if (k == 0) { hdr[2] = koff[P.m + 1]; return; }
    const u32 d = koff[k];
    if (koff[k + 1] == d) return;
    const u32 r = perm[k - 1];
    if (r >= P.n || d >= P.n) return;
    const GlcList &L = P.L;
    W.s1[d] = L.s1[r]; W.e1[d] = L.e1[r]; W.s2[d] = L.s2[r]; W.e2[d] = L.e2[r]; W.score[d] = L.score[r];
    W.o[d] = L.o[r]; W.refid[d] = L.refid[r]; W.ctgid[d] = L.ctgid[r]; W.idx[d] = L.idx[r];
}

int bits_of(u64 v) { int b = 0; while (v) { b++; v >>= 1; } return b ? b : 1; }

struct Events {
    std::vector<hipEvent_t> ev;
    ~Events() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }
    hipEvent_t get(size_t k) { while (ev.size() <= k) { hipEvent_t e = nullptr; if (hipEventCreate(&e) != hipSuccess) return nullptr; ev.push_back(e); } return ev[k]; }
};

void info_pass(int64_t *info, int ninfo, int axis, int64_t left) {
    if (!info) return;
    info[axis ? RV_GLC_PASSES1 : RV_GLC_PASSES0]++;
    const int64_t k = info[RV_GLC_NAFTER]++;
    if (RV_GLC_INFO_HEAD + k < ninfo) info[RV_GLC_INFO_HEAD + k] = left;
}

// the dummies of an axis: positions of the sequence ends, `start` at the first sequence's begin (transform.py:951-970)
int dummies(const RvGlcIn &in, int axis, std::vector<int64_t> &pos, int64_t &startpos) {
    pos.clear();
    bool have = false;
    for (int64_t i = 0; i < in.nseq; i++) {
        const bool ref = in.rs[i] < in.sep;
        if (ref != (axis == 0)) continue;
        if (!have) { startpos = in.rs[i]; have = true; }
        pos.push_back(in.re[i]);
    }
    if (!have) { rv_set_error("glocalchain: no sequence on axis %d", axis); return -1; }
    return 0;
}

}  // namespace

int rv_glocal_admit_rule(int64_t n, int64_t nseq, int64_t maxcoord, int64_t maxscore, const RvGlcParams &w) {
    if (w.rearr < 0 || w.inv < 0 || w.lambda < 0 || w.eps < 0 || w.alfa < 0 || w.gapopen < 0) { rv_set_error("glocalchain: negative weight"); return -1; }
    if (n < 0 || nseq < 0 || maxcoord < 0 || maxscore < 0) { rv_set_error("glocalchain: bad arguments"); return -1; }
    typedef __int128 i128;
    const i128 lim = (i128)1 << 62;
    const i128 span = 2 * (i128)maxcoord + 2;                                 // no difference of two coordinates, and no sum of two such, is larger
    if ((i128)w.lambda * span >= lim || (i128)w.eps * span >= lim) return 0;
    const i128 step = (i128)w.alfa * maxscore + (i128)w.gapopen + 2 * (i128)w.rearr + (i128)w.inv + (i128)w.eps * span;      // one block's gain and one edge's cost
    return step * ((i128)n + nseq + 2) < lim ? 1 : 0;
}

int rv_glocal_validate(const RvGlcIn &in, int64_t *maxcoord, int64_t *maxscore) {
    if (in.n < 0 || in.nseq <= 0 || !in.rs || !in.re || (in.n && (!in.s1 || !in.e1 || !in.s2 || !in.e2 || !in.o || !in.score || !in.refid || !in.ctgid))) {
        rv_set_error("glocalchain: bad arguments"); return -1;
    }
    if (in.n > 0x7ffffff0ll - in.nseq) { rv_set_error("glocalchain: more than 2^31 - 16 entries"); return -1; }
    const int64_t lim = (int64_t)1 << 61;
    int64_t mc = 0, ms = 0, nref = 0;
    for (int64_t i = 0; i < in.nseq; i++) {
        if (in.rs[i] < 0 || in.rs[i] > in.re[i] || in.re[i] >= lim || (i && in.rs[i] <= in.re[i - 1])) { rv_set_error("glocalchain: ctg2range is not a list of ascending ranges inside 0 .. 2^61"); return -1; }
        if (in.rs[i] < in.sep) { if (nref != i) { rv_set_error("glocalchain: a reference sequence behind a contig"); return -1; } nref++; }
        mc = std::max(mc, in.re[i]);
    }
    for (int64_t i = 0; i < in.n; i++) {
        if (in.s1[i] < 0 || in.s2[i] < 0 || in.s1[i] > in.e1[i] || in.s2[i] > in.e2[i] || in.e1[i] >= lim || in.e2[i] >= lim) { rv_set_error("glocalchain: block %lld: coordinates outside 0 <= s <= e < 2^61", (long long)i); return -1; }
        if (in.o[i] != 0 && in.o[i] != 1) { rv_set_error("glocalchain: block %lld: orientation is 0 or 1", (long long)i); return -1; }
        if (in.score[i] < 0 || in.score[i] >= lim) { rv_set_error("glocalchain: block %lld: score outside 0 .. 2^61", (long long)i); return -1; }
        if (in.refid[i] < 0 || in.refid[i] >= nref) { rv_set_error("glocalchain: block %lld: refid names no reference sequence", (long long)i); return -1; }
        if (in.ctgid[i] < nref || in.ctgid[i] >= in.nseq) { rv_set_error("glocalchain: block %lld: ctgid names no contig", (long long)i); return -1; }
        mc = std::max(mc, std::max(in.e1[i], in.e2[i])); ms = std::max(ms, in.score[i]);
    }
    *maxcoord = mc; *maxscore = ms;
    return 0;
}

// ---- the host programme: the same rule, std::stable_sort and the reference's loop ------------------------------------------------------------------------
static int glc_host_pass(const RvGlcIn &in, const RvGlcParams &w, int axis, const std::vector<int32_t> &cur, std::vector<int32_t> &next) {
    next.clear();
    const size_t n = cur.size();
    if (n == 0) return 0;
    std::vector<int64_t> dpos; int64_t startpos = 0;
    if (dummies(in, axis, dpos, startpos) != 0) return -1;
    const size_t m = n + dpos.size();
    std::vector<GlcEntry> ent(m);
    std::vector<int64_t> sc(m, 0);
    for (size_t i = 0; i < n; i++) {
        const int32_t r = cur[i];
        GlcEntry &e = ent[i];
        if (axis == 0) { e.a = in.s1[r]; e.ae = in.e1[r]; e.b = in.s2[r]; e.be = in.e2[r]; e.id1 = in.refid[r]; e.id2 = in.ctgid[r]; }
        else { e.a = in.s2[r]; e.ae = in.e2[r]; e.b = in.s1[r]; e.be = in.e1[r]; e.id1 = in.ctgid[r]; e.id2 = in.refid[r]; }
        e.o = in.o[r]; sc[i] = in.score[r];
    }
    for (size_t i = n; i < m; i++) { GlcEntry &e = ent[i]; e.a = e.ae = dpos[i - n]; e.b = e.be = 0; e.o = 0; e.id1 = e.id2 = -1; }
    std::vector<u32> ord(m);
    std::iota(ord.begin(), ord.end(), 0u);
    std::stable_sort(ord.begin(), ord.end(), [&](u32 x, u32 y) { return ent[x].a != ent[y].a ? ent[x].a < ent[y].a : sc[x] > sc[y]; });
    std::vector<GlcEntry> H(m + 1);
    H[0].a = H[0].ae = startpos; H[0].b = H[0].be = 0; H[0].o = 0; H[0].id1 = H[0].id2 = -1;
    size_t kend = 0;
    for (size_t k = 1; k <= m; k++) { H[k] = ent[ord[k - 1]]; if (ord[k - 1] == m - 1) kend = k; }
    std::vector<int64_t> score(m + 1, 0);
    std::vector<u32> back(m + 1, 0);
    size_t deepest = 1;
    for (size_t k = 1; k <= m; k++) {
        const GlcEntry &b = H[k];
        while (H[deepest].ae < b.a) deepest++;
        const int64_t da = H[deepest].a;
        bool have = false; int64_t best = 0, l = 0; u32 bp = 0;
        for (size_t p = k; p-- > 0;) {
            const GlcEntry &q = H[p];
            if (glc_skip(q.a, q.ae, q.b, q.be, q.id1, b.a, b.ae, b.b, b.be, b.id1)) continue;
            l++;
            const int64_t v = score[p] - glc_cost(q, b, axis, w, in.rs, in.re);
            if (!have || v > best) { have = true; best = v; bp = (u32)p; }
            if (b.a - q.a > w.lastbp && l >= w.lastn && q.a < da) break;
        }
        score[k] = best + w.alfa * sc[ord[k - 1]];
        back[k] = bp;
    }
    for (u32 node = back[kend]; node != 0; node = back[node])
        if (H[node].id1 >= 0) next.push_back(cur[ord[node - 1]]);
    std::reverse(next.begin(), next.end());
    return 0;
}

int rv_glocal_rule_host(const RvGlcIn &in, const RvGlcParams &w, int axes, int fixed, int64_t *info, int ninfo, RvGlcOut &out) {
    out.clear();
    if (info) { for (int k = 0; k < ninfo; k++) info[k] = 0; if (ninfo < RV_GLC_INFO_HEAD) info = nullptr; }
    if (!(axes & 3) || (axes & ~3)) { rv_set_error("glocalchain: axes names the reference axis (1), the query axis (2) or both (3)"); return -1; }
    int64_t mc = 0, ms = 0;
    if (rv_glocal_validate(in, &mc, &ms) != 0) return -1;
    const int adm = rv_glocal_admit_rule(in.n, in.nseq, mc, ms, w);
    if (adm < 0) return -1;
    if (!adm) { rv_set_error("glocalchain: these weights may leave 62 bits on this list (rv_glocal_admit)"); return -1; }
    if (info) info[RV_GLC_ROUTE] = 1;
    try {
        std::vector<int32_t> cur((size_t)in.n), next;
        std::iota(cur.begin(), cur.end(), 0);
        for (int axis = 0; axis < 2; axis++) {
            if (!(axes >> axis & 1)) continue;
            for (;;) {
                if (glc_host_pass(in, w, axis, cur, next) != 0) return -1;
                const bool dropped = next.size() != cur.size();
                cur.swap(next);
                info_pass(info, ninfo, axis, (int64_t)cur.size());
                if (!fixed || !dropped) break;
            }
        }
        out.idx = cur;
    } catch (...) { rv_set_error("glocalchain: out of host memory"); return -1; }
    return 0;
}

// ---- the device programme ---------------------------------------------------------------------------------------------------------------------------------------
int rv_glocal_device(Workspace &ws, const RvGlcIn &in, const RvGlcParams &w, int axes, int fixed, int64_t *info, int ninfo, RvGlcOut &out) {
    out.clear();
    if (info) { for (int k = 0; k < ninfo; k++) info[k] = 0; if (ninfo < RV_GLC_INFO_HEAD) info = nullptr; }
    if (!(axes & 3) || (axes & ~3)) { rv_set_error("glocalchain: axes names the reference axis (1), the query axis (2) or both (3)"); return -1; }
    int64_t mc = 0, ms = 0;
    if (rv_glocal_validate(in, &mc, &ms) != 0) return -1;
    const int adm = rv_glocal_admit_rule(in.n, in.nseq, mc, ms, w);
    if (adm < 0) return -1;
    if (!adm) { rv_set_error("glocalchain: these weights may leave 62 bits on this list (rv_glocal_admit)"); return -1; }
    std::vector<int64_t> dpos[2]; int64_t startpos[2] = {0, 0};
    for (int axis = 0; axis < 2; axis++)
        if ((axes >> axis & 1) && dummies(in, axis, dpos[axis], startpos[axis]) != 0) return -1;
    if (in.n == 0) {
        for (int axis = 0; axis < 2; axis++) if (axes >> axis & 1) info_pass(info, ninfo, axis, 0);
        return 0;
    }
    hipStream_t q = ws.stream;
    const size_t n0 = (size_t)in.n, nseq = (size_t)in.nseq;
    const size_t m0 = n0 + std::max(dpos[0].size(), dpos[1].size()), M2 = m0 + 2;
    // one arena for everything that scales with the list, 256-byte aligned pieces
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += (bytes + 255) & ~(size_t)255; return o; };
    const size_t oL0 = take(n0 * GLC_LIST_BYTES), oL1 = take(n0 * GLC_LIST_BYTES), oKa = take(m0 * 8), oKb = take(m0 * 8), oVa = take(m0 * 4), oVb = take(m0 * 4);
    const size_t oH = take(M2 * (5 * 8 + 3 * 4)), oEnds = take(M2 * 8), oRmax = take(M2 * 8), oEoff = take(M2 * 8), oScore = take(M2 * 8), oBack = take(M2 * 4);
    const size_t oJ0 = take(M2 * 4), oJ1 = take(M2 * 4), oM = take(M2 * 4);
    RV_TRY(ws.glc[0].reserve(at));
    char *A = ws.glc[0].as<char>();
    // the tables that stay for every pass: ranges, the dummies of both axes, the header
    const size_t tbytes = (2 * nseq + dpos[0].size() + dpos[1].size()) * 8 + 64;
    RV_TRY(ws.glc[2].reserve(tbytes));
    int64_t *d_rs = ws.glc[2].as<int64_t>(), *d_re = d_rs + nseq, *d_dp[2] = {d_re + nseq, d_re + nseq + dpos[0].size()};
    u32 *hdr = (u32 *)(d_dp[1] + dpos[1].size());
    RV_HIP(hipMemcpyAsync(d_rs, in.rs, nseq * 8, hipMemcpyHostToDevice, q));
    RV_HIP(hipMemcpyAsync(d_re, in.re, nseq * 8, hipMemcpyHostToDevice, q));
    for (int axis = 0; axis < 2; axis++)
        if (!dpos[axis].empty()) RV_HIP(hipMemcpyAsync(d_dp[axis], dpos[axis].data(), dpos[axis].size() * 8, hipMemcpyHostToDevice, q));
    GlcList L[2] = {GlcList(A + oL0, n0), GlcList(A + oL1, n0)};
    std::vector<int32_t> iota;
    try { iota.resize(n0); std::iota(iota.begin(), iota.end(), 0); } catch (...) { rv_set_error("glocalchain: out of host memory"); return -1; }
    RV_HIP(hipMemcpyAsync(L[0].s1, in.s1, n0 * 8, hipMemcpyHostToDevice, q)); RV_HIP(hipMemcpyAsync(L[0].e1, in.e1, n0 * 8, hipMemcpyHostToDevice, q));
    RV_HIP(hipMemcpyAsync(L[0].s2, in.s2, n0 * 8, hipMemcpyHostToDevice, q)); RV_HIP(hipMemcpyAsync(L[0].e2, in.e2, n0 * 8, hipMemcpyHostToDevice, q));
    RV_HIP(hipMemcpyAsync(L[0].score, in.score, n0 * 8, hipMemcpyHostToDevice, q)); RV_HIP(hipMemcpyAsync(L[0].o, in.o, n0 * 4, hipMemcpyHostToDevice, q));
    RV_HIP(hipMemcpyAsync(L[0].refid, in.refid, n0 * 4, hipMemcpyHostToDevice, q)); RV_HIP(hipMemcpyAsync(L[0].ctgid, in.ctgid, n0 * 4, hipMemcpyHostToDevice, q));
    RV_HIP(hipMemcpyAsync(L[0].idx, iota.data(), n0 * 4, hipMemcpyHostToDevice, q));
    RV_HIP(hipStreamSynchronize(q));      // (the host arrays are the caller's)
    if (info) info[RV_GLC_BYTES_UP] = (int64_t)(n0 * GLC_LIST_BYTES + tbytes - 64);
    GlcH H;
    {
        char *p = A + oH;
        H.a = (int64_t *)p; H.ae = H.a + M2; H.b = H.ae + M2; H.be = H.b + M2; H.sc = H.be + M2; H.o = (int32_t *)(H.sc + M2); H.id1 = H.o + M2; H.id2 = H.id1 + M2;
    }
    u64 *ends = (u64 *)(A + oEnds), *rmax = (u64 *)(A + oRmax), *eoff = (u64 *)(A + oEoff);
    int64_t *score = (int64_t *)(A + oScore);
    u32 *back = (u32 *)(A + oBack), *J[2] = {(u32 *)(A + oJ0), (u32 *)(A + oJ1)}, *M = (u32 *)(A + oM);
    const int pbits = bits_of((u64)mc), sbits = bits_of((u64)ms);
    const u64 budget = (u64)std::max<int64_t>(ws.opt.glocal_edge_budget, 1);
    Events events;
    int cur = 0;
    size_t n = n0;
    for (int axis = 0; axis < 2; axis++) {
        if (!(axes >> axis & 1)) continue;
        for (;;) {
            if (n == 0) { info_pass(info, ninfo, axis, 0); break; }
            GlcPass P;
            P.L = L[cur]; P.n = (u32)n; P.nd = (u32)dpos[axis].size(); P.m = P.n + P.nd; P.dpos = d_dp[axis]; P.startpos = startpos[axis]; P.axis = axis;
            const u32 m = P.m;
            const unsigned gm = (unsigned)ceil_div((int64_t)m + 2, 256);
            u64 *ka = (u64 *)(A + oKa), *kb = (u64 *)(A + oKb);
            u32 *va = (u32 *)(A + oVa), *vb = (u32 *)(A + oVb);
            int f = 0;
            RV_HIP(hipMemsetAsync(hdr, 0, 16, q));
            if (pbits + sbits <= 64) {
                hipLaunchKernelGGL(k_glc_keys, dim3(gm), dim3(256), 0, q, P, 0, sbits, ms, (const u32 *)nullptr, ka, va);
                RV_LAUNCH_CHECK();
                RV_TRY(rv_radix_sort_pairs<u32>(ws, ka, va, kb, vb, (int64_t)m, 0, pbits + sbits, &f));
                if (f) { std::swap(ka, kb); std::swap(va, vb); }
            } else {
                hipLaunchKernelGGL(k_glc_keys, dim3(gm), dim3(256), 0, q, P, 1, 0, ms, (const u32 *)nullptr, ka, va);
                RV_LAUNCH_CHECK();
                RV_TRY(rv_radix_sort_pairs<u32>(ws, ka, va, kb, vb, (int64_t)m, 0, sbits, &f));
                if (f) { std::swap(ka, kb); std::swap(va, vb); }
                hipLaunchKernelGGL(k_glc_keys, dim3(gm), dim3(256), 0, q, P, 2, 0, ms, (const u32 *)va, kb, vb);
                RV_LAUNCH_CHECK();
                RV_TRY(rv_radix_sort_pairs<u32>(ws, kb, vb, ka, va, (int64_t)m, 0, pbits, &f));
                if (!f) { std::swap(ka, kb); std::swap(va, vb); }
            }
            if (info) info[RV_GLC_SORT_KEYS] = pbits + sbits <= 64 ? 1 : 2;
            const u32 *perm = va;
            hipLaunchKernelGGL(k_glc_gather, dim3(gm), dim3(256), 0, q, P, perm, H, ends, score, back, hdr);
            RV_LAUNCH_CHECK();
            RV_TRY(rv_inclusive_max_u64(ws, ends, rmax, (int64_t)m + 1));
            hipLaunchKernelGGL(k_glc_window, dim3(gm), dim3(256), 0, q, H, (const u64 *)rmax, m, w.lastn, w.lastbp, eoff, hdr);
            RV_LAUNCH_CHECK();
            RV_TRY(rv_exclusive_sum_u64(ws, eoff, eoff, (int64_t)m + 2));
            u32 hh[4] = {0, 0, 0, 0}; u64 total = 0;
            RV_TRY(rv_read_back2(ws, hh, hdr, 16, &total, eoff + m + 1, 8));
            if (hh[0] < 1 || hh[0] > m || hh[1] < 1 || hh[1] > m || total < m || total > (u64)m * hh[1]) { rv_set_error("glocalchain: inconsistent counts from the device"); return -1; }
            const u64 ntiles = total / budget + 1, ecap = std::min(total, budget + hh[1]);
            RV_TRY(ws.glc[1].reserve((size_t)ecap * 8));
            int64_t *E = ws.glc[1].as<int64_t>();
            const unsigned ge = (unsigned)ceil_div((int64_t)ecap, 256);
            size_t timed = 0;
            for (u64 t = 0; t < ntiles; t++) {
                hipLaunchKernelGGL(k_glc_cost, dim3(ge), dim3(256), 0, q, H, (const u64 *)eoff, m, t, budget, axis, w, (const int64_t *)d_rs, (const int64_t *)d_re, E, ecap);
                RV_LAUNCH_CHECK();
                hipEvent_t e0 = timed < 32 ? events.get(2 * timed) : nullptr, e1 = e0 ? events.get(2 * timed + 1) : nullptr;
                if (e1) RV_HIP(hipEventRecord(e0, q));
                hipLaunchKernelGGL(k_glc_chain, dim3(1), dim3(64), 0, q, (const u64 *)eoff, (const int64_t *)H.sc, m, t, budget, w.alfa, (const int64_t *)E, ecap, score, back);
                RV_LAUNCH_CHECK();
                if (e1) { RV_HIP(hipEventRecord(e1, q)); timed++; }
            }
            // the path from `end`
            hipLaunchKernelGGL(k_glc_mark_init, dim3(gm), dim3(256), 0, q, m, (const u32 *)hdr, M);
            RV_LAUNCH_CHECK();
            const u32 *jin = back; int jo = 0;
            for (u64 reach = 1; reach < (u64)m + 1; reach <<= 1) {
                hipLaunchKernelGGL(k_glc_double, dim3(gm), dim3(256), 0, q, m, jin, J[jo], M);
                RV_LAUNCH_CHECK();
                jin = J[jo]; jo ^= 1;
            }
            hipLaunchKernelGGL(k_glc_keep, dim3(gm), dim3(256), 0, q, m, (const int32_t *)H.id1, M);
            RV_LAUNCH_CHECK();
            RV_TRY(rv_exclusive_sum_u32(ws, M, M, (int64_t)m + 2));
            hipLaunchKernelGGL(k_glc_compact, dim3(gm), dim3(256), 0, q, P, perm, (const u32 *)M, L[cur ^ 1], hdr);
            RV_LAUNCH_CHECK();
            u32 left = 0;
            RV_TRY(rv_read_back(ws, &left, hdr + 2, 4));
            if (left > n) { rv_set_error("glocalchain: inconsistent counts from the device"); return -1; }
            if (info) {
                info[RV_GLC_TILES] += (int64_t)ntiles; info[RV_GLC_TILES_MAX] = std::max(info[RV_GLC_TILES_MAX], (int64_t)ntiles);
                info[RV_GLC_EDGES] += (int64_t)total; info[RV_GLC_BYTES_DOWN] += 28;
                for (size_t k = 0; k < timed; k++) { float ms_ = 0; if (hipEventElapsedTime(&ms_, events.ev[2 * k], events.ev[2 * k + 1]) == hipSuccess) info[RV_GLC_CHAIN_NS] += (int64_t)((double)ms_ * 1e6); }
                if (timed == ntiles) info[RV_GLC_CHAIN_BLOCKS] += m;
            }
            const bool dropped = left != n;
            n = left; cur ^= 1;
            info_pass(info, ninfo, axis, (int64_t)n);
            if (!fixed || !dropped) break;
        }
    }
    try { out.idx.resize(n); } catch (...) { rv_set_error("glocalchain: out of host memory"); return -1; }
    if (n) {
        RV_HIP(hipMemcpyAsync(out.idx.data(), L[cur].idx, n * 4, hipMemcpyDeviceToHost, q));
        RV_HIP(hipStreamSynchronize(q));
        if (info) info[RV_GLC_BYTES_DOWN] += (int64_t)n * 4;
    }
    return 0;
}
