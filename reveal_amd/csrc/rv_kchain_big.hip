// rv_kchain_big.hip -- the chaining programme of rv_kchain.hip (reveal/chain.py:269-289) for lists above the caps of k_many_kchain, in device memory.
// The host prepares a list as for rv_kchain (kc_prepare: the cap, the points, the order of the targets, the kd order) and uploads it in TARGET order:
// point i is the i-th target.  A candidate of a target lies strictly in front of it in dimension 0 (its length is at least 1 and no two points share
// a coordinate), so it has a smaller index.  The targets are cut into tiles of RV_KCHAIN_BIG_TILE = T; k_kchain_big_step(b) is step b of every list:
//   push      the workgroup of every tile behind b loads tile b -- final since step b - 1 -- into LDS; each thread owns one target and offers it the T
//             points: admissible in every dimension, score_v + wscore l_v k(k-1)/2 - wpen gapcost(v, t), kept when greater or equal with the smaller
//             kd rank.  One thread owns a target, so there is no atomic; the running best (score, kd rank, index) lies in device memory between steps
//   diagonal  the workgroup of tile b + 1 then finishes its tile: point after point becomes final (p1's offer -wpen gapcost(p1, t) stays unless an
//             offer is strictly greater) and is pushed to the points behind it in the tile.  With T = 64 the workgroup is one wavefront
// Step -1 is the diagonal of tile 0.  The order between the tiles is the order of the launches on the stream: no workgroup waits for another, and a list
// whose tiles are exhausted does nothing.  Several lists share the launches (grid dimension y), so their number is the tiles of the longest list.
// Three forms by k: 2 (the target's coordinates in two registers), 3 .. 8 (both tiles' coordinates in LDS), 9 .. 64 (coordinates read where they lie).
#include "../../include/reveal_amd.h"
#include "rv_kchain_big.h"
#include <algorithm>
#include <climits>

namespace {

constexpr int BT = RV_KCHAIN_BIG_TILE;
static_assert(BT == 64 || BT == 128 || BT == 256, "a tile is one to four wavefronts");
constexpr u32 BNONE = 0xFFFFFFFFu;
constexpr int BLISTS = 65535;      // lists of one run: grid dimension y

struct KcBigDesc { u64 o, co; u32 n1, k; };      // a list: its first point, its first coordinate (P[co + d n1 + i]), points with p2, sequences
struct KcBigArgs {
    const KcBigDesc *lists; int nlists;
    const u32 *P, *L, *kdr; u64 npts, ncoord;
    int64_t *bs; u32 *bk, *bv;        // the running best offer of a point: score, kd rank and index of the offerer (BNONE: none)
    int64_t *score; u32 *back;        // final
    u32 *err;                         // bit 1 a list outside its room, 4 a back-pointer outside its list
    int64_t wpen, wscore; int model;
};
struct KcBigShared {
    u32 cP[8 * BT], oP[8 * BT];       // coordinates of tile b and of the workgroup's own tile, dimension-major (k <= 8)
    u32 cL[BT], cK[BT], oL[BT], oK[BT];
    int64_t cS[BT], oS[BT];
};
struct KcPair { u32 a, b; __device__ int64_t operator()(int i) const { return (int64_t)(i ? b : a); } };

template <class CA, class TA>
__device__ inline void kc_big_offer(const CA &ca, const TA &ta, int k, u32 lv, u32 kv, int64_t sv, u32 iv, const KcBigArgs &A, int64_t gain, int64_t &bs, u32 &bk, u32 &bv) {
    for (int d = 0; d < k; d++) if (ca(d) + (int64_t)lv > ta(d)) return;
    const int64_t sc = sv + A.wscore * ((int64_t)lv * gain) - A.wpen * kc_gap(ca, ta, k, A.model);
    if (sc > bs || (sc == bs && kv < bk)) { bs = sc; bk = kv; bv = iv; }
}

template <int KM, class TA>
__device__ inline void kc_big_tile(KcBigShared &S, const KcBigArgs &A, const KcBigDesc &D, const TA &ta, int b, u32 tile, bool live, u32 i) {
    const int tid = (int)threadIdx.x, k = (int)D.k;
    const u32 n1 = D.n1;
    const u32 *Pl = A.P + D.co;
    const u64 g = D.o + i;
    const int64_t gain = (int64_t)(k * (k - 1) / 2);
    int64_t bs = INT64_MIN;
    u32 bk = BNONE, bv = BNONE;
    if (b >= 1 && live) { bs = A.bs[g]; bk = A.bk[g]; bv = A.bv[g]; }      // (step 0 is the first push a tile sees)
    if (b >= 0 && live) {
        const u32 c0 = (u32)b * BT;      // (tile b is whole: a tile behind it exists)
        for (int v = 0; v < BT; v++) {
            if constexpr (KM <= 8) kc_big_offer(KcStrided{S.cP + v, BT}, ta, k, S.cL[v], S.cK[v], S.cS[v], c0 + (u32)v, A, gain, bs, bk, bv);
            else kc_big_offer(KcStrided{Pl + c0 + v, (int64_t)n1}, ta, k, S.cL[v], S.cK[v], S.cS[v], c0 + (u32)v, A, gain, bs, bk, bv);
        }
    }
    if (tile != (u32)(b + 1)) {
        if (live) { A.bs[g] = bs; A.bk[g] = bk; A.bv[g] = bv; }
        return;
    }
    // the diagonal: point v of the tile becomes final, then offers itself to the points behind it
    const u32 t0 = tile * BT;
    const int cnt = (int)(n1 - t0 < (u32)BT ? n1 - t0 : (u32)BT);
    const int64_t ps = live ? -A.wpen * kc_gap(KcP1(), ta, k, A.model) : 0;
    for (int v = 0; v < cnt; v++) {
        if (tid == v) {
            const bool take = bk != BNONE && bs > ps;      // strict: p1 stays where nothing beats it
            u32 fb = take ? bv : BNONE;
            if (fb != BNONE && fb >= i) { atomicOr(A.err, 4u); fb = BNONE; }      // (an offerer lies in front of its target)
            const int64_t fs = take ? bs : ps;
            A.score[g] = fs; A.back[g] = fb; S.oS[v] = fs;
        }
        __syncthreads();
        if (tid > v && live) {
            if constexpr (KM <= 8) kc_big_offer(KcStrided{S.oP + v, BT}, ta, k, S.oL[v], S.oK[v], S.oS[v], t0 + (u32)v, A, gain, bs, bk, bv);
            else kc_big_offer(KcStrided{Pl + t0 + v, (int64_t)n1}, ta, k, S.oL[v], S.oK[v], S.oS[v], t0 + (u32)v, A, gain, bs, bk, bv);
        }
    }
}

__global__ __launch_bounds__(BT) void k_kchain_big_step(KcBigArgs A, int b) {
    __shared__ KcBigShared S;
    const int tid = (int)threadIdx.x;
    if ((int)blockIdx.y >= A.nlists) return;
    const KcBigDesc D = A.lists[blockIdx.y];
    if (!(D.k >= 2 && D.k <= 64 && D.n1 >= 2 && (u64)D.n1 <= (u64)RV_KCHAIN_BIG_CAP + 1 && D.o <= A.npts && (u64)D.n1 <= A.npts - D.o && D.co <= A.ncoord &&
          (u64)D.n1 * D.k <= A.ncoord - D.co)) {
        if (tid == 0) atomicOr(A.err, 1u);
        return;
    }
    const u64 tile64 = (u64)(b + 1) + blockIdx.x;
    if (b < -1 || tile64 * BT >= (u64)D.n1) return;      // (the list's tiles are exhausted)
    const u32 tile = (u32)tile64, n1 = D.n1, i = tile * BT + (u32)tid;
    const int k = (int)D.k;
    const bool live = i < n1;
    const u32 *Pl = A.P + D.co;
    if (live) {
        if (k <= 8) for (int d = 0; d < k; d++) S.oP[d * BT + tid] = Pl[(u64)d * n1 + i];
        S.oL[tid] = A.L[D.o + i]; S.oK[tid] = A.kdr[D.o + i];
    }
    if (b >= 0) {
        const u32 cv = (u32)b * BT + (u32)tid;      // (< n1: tile b lies in front of this one)
        if (k <= 8) for (int d = 0; d < k; d++) S.cP[d * BT + tid] = Pl[(u64)d * n1 + cv];
        S.cL[tid] = A.L[D.o + cv]; S.cK[tid] = A.kdr[D.o + cv]; S.cS[tid] = A.score[D.o + cv];
    }
    __syncthreads();
    if (k == 2) kc_big_tile<2>(S, A, D, KcPair{live ? S.oP[tid] : 0u, live ? S.oP[BT + tid] : 0u}, b, tile, live, i);
    else if (k <= 8) kc_big_tile<8>(S, A, D, KcStrided{S.oP + tid, BT}, b, tile, live, i);
    else kc_big_tile<64>(S, A, D, KcStrided{Pl + (live ? i : 0u), (int64_t)n1}, b, tile, live, i);
}

}  // namespace

int rv_kchain_big_run(Workspace &ws, RvKchainBigBufs &B, const std::vector<const KcPrep *> &lists, int64_t wpen, int64_t wscore, int gcmodel,
                      std::vector<std::vector<int64_t>> &score, std::vector<std::vector<int>> &back, int64_t *launches) {
    const size_t nl = lists.size();
    score.assign(nl, std::vector<int64_t>());
    back.assign(nl, std::vector<int>());
    if (nl == 0) return 0;
    if (nl > (size_t)BLISTS) {      // (more lists than a grid holds: runs of BLISTS)
        for (size_t lo = 0; lo < nl; lo += BLISTS) {
            const size_t hi = std::min(nl, lo + (size_t)BLISTS);
            std::vector<const KcPrep *> part(lists.begin() + (ptrdiff_t)lo, lists.begin() + (ptrdiff_t)hi);
            std::vector<std::vector<int64_t>> ps;
            std::vector<std::vector<int>> pb;
            RV_TRY(rv_kchain_big_run(ws, B, part, wpen, wscore, gcmodel, ps, pb, launches));
            for (size_t x = lo; x < hi; x++) { score[x].swap(ps[x - lo]); back[x].swap(pb[x - lo]); }
        }
        return 0;
    }
    std::vector<KcBigDesc> desc(nl);
    u64 npts = 0, ncoord = 0;
    u32 nmax = 0;
    for (size_t x = 0; x < nl; x++) {
        const KcPrep &pp = *lists[x];
        if (pp.refuse || pp.m < 1 || pp.k < 2 || pp.k > 64 || (int64_t)pp.m > RV_KCHAIN_BIG_CAP || pp.order.size() != (size_t)pp.m + 1 || pp.kd.size() != (size_t)pp.m + 1) {
            rv_set_error("rv_kchain_big: a list the preparation has not admitted");
            return -1;
        }
        desc[x].o = npts; desc[x].co = ncoord; desc[x].n1 = (u32)pp.m + 1; desc[x].k = (u32)pp.k;
        npts += (u64)pp.m + 1; ncoord += ((u64)pp.m + 1) * (u64)pp.k;
        nmax = std::max(nmax, desc[x].n1);
    }
    // P | L | kdr, every list in target order
    std::vector<u32> hin((size_t)(ncoord + 2 * npts));
    u32 *hP = hin.data(), *hL = hP + ncoord, *hK = hL + npts;
    for (size_t x = 0; x < nl; x++) {
        const KcPrep &pp = *lists[x];
        const size_t n1 = (size_t)pp.m + 1, k = (size_t)pp.k;
        std::vector<u32> rank_kd(n1, BNONE);
        for (size_t q = 0; q < n1; q++) {
            const int p = pp.kd[q];
            if (p < 0 || (size_t)p >= n1 || rank_kd[(size_t)p] != BNONE) { rv_set_error("rv_kchain_big: the kd order is no permutation"); return -1; }
            rank_kd[(size_t)p] = (u32)q;
        }
        for (size_t r = 0; r < n1; r++) {
            const int p = pp.order[r];
            if (p < 0 || (size_t)p >= n1) { rv_set_error("rv_kchain_big: the target order is no permutation"); return -1; }
            for (size_t d = 0; d < k; d++) hP[desc[x].co + d * n1 + r] = (u32)pp.P[(size_t)p * k + d];
            hL[desc[x].o + r] = (u32)pp.L[(size_t)p];
            hK[desc[x].o + r] = rank_kd[(size_t)p];
        }
    }
    const size_t in_bytes = hin.size() * sizeof(u32), st_bytes = (size_t)npts * 16, o_back = (size_t)npts * 8, o_err = o_back + (((size_t)npts + 1) / 2) * 8,
                 out_bytes = o_err + 8;
    RV_TRY(B.in.reserve(in_bytes));
    RV_TRY(B.state.reserve(st_bytes));
    RV_TRY(B.out.reserve(out_bytes));
    RV_TRY(B.lists.reserve(nl * sizeof(KcBigDesc)));
    hipStream_t q = ws.stream;
    RV_HIP(hipMemcpyAsync(B.in.p, hin.data(), in_bytes, hipMemcpyHostToDevice, q));
    RV_HIP(hipMemcpyAsync(B.lists.p, desc.data(), nl * sizeof(KcBigDesc), hipMemcpyHostToDevice, q));
    RV_HIP(hipMemsetAsync((char *)B.out.p + o_back, 0, out_bytes - o_back, q));
    KcBigArgs A;
    A.lists = (const KcBigDesc *)B.lists.p; A.nlists = (int)nl;
    A.P = (const u32 *)B.in.p; A.L = A.P + ncoord; A.kdr = A.L + npts; A.npts = npts; A.ncoord = ncoord;
    A.bs = (int64_t *)B.state.p; A.bk = (u32 *)(A.bs + npts); A.bv = A.bk + npts;
    A.score = (int64_t *)B.out.p; A.back = (u32 *)((char *)B.out.p + o_back); A.err = (u32 *)((char *)B.out.p + o_err);
    A.wpen = wpen; A.wscore = wscore; A.model = gcmodel;
    const int ntiles = (int)(((u64)nmax + BT - 1) / BT);
    for (int b = -1; b + 1 < ntiles; b++) {
        hipLaunchKernelGGL(k_kchain_big_step, dim3((unsigned)(b < 0 ? 1 : ntiles - 1 - b), (unsigned)nl), dim3(BT), 0, q, A, b);
        RV_LAUNCH_CHECK();
        if (launches) *launches += 1;
    }
    std::vector<u64> hout(out_bytes / 8);
    RV_TRY(rv_read_back(ws, hout.data(), B.out.p, out_bytes));
    u32 err = 0;
    memcpy(&err, (const char *)hout.data() + o_err, 4);
    if (err) { rv_set_error("rv_kchain_big: the step kernel met an index outside its room (error bits %u: 1 list, 4 back-pointer)", err); return -1; }
    const int64_t *hs = (const int64_t *)hout.data();
    const u32 *hb = (const u32 *)((const char *)hout.data() + o_back);
    for (size_t x = 0; x < nl; x++) {
        const KcPrep &pp = *lists[x];
        const size_t n1 = (size_t)pp.m + 1;
        score[x].assign(n1, 0); back[x].assign(n1, -1);
        for (size_t r = 0; r < n1; r++) {
            const size_t p = (size_t)pp.order[r];
            const u32 v = hb[desc[x].o + r];
            if (v != BNONE && v >= n1) { rv_set_error("rv_kchain_big: a back-pointer outside its list"); return -1; }
            score[x][p] = hs[desc[x].o + r];
            back[x][p] = v == BNONE ? -1 : pp.order[(size_t)v];
        }
    }
    return 0;
}
