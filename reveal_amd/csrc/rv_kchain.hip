// rv_kchain.hip -- the collinear chain of `reveal chain` (reveal/chain.py:214-314 `chain()`, utils.py:162-183 `gapcost`, :983-1033 `kdtree` / `range_search`)
// for the jobs of rv_many: what `reveal chain --recurse` does with the getmultimums(minn = k) list of the fresh index of every gap.  DESIGN.md 3j has the
// algorithm as kept and the argument for the "kd order": candidates of equal score are decided by the order in which range_search hands them out, the
// right-first depth-first leaf order of kdtree(points, k) -- ONE total order of the points, whatever the query, since a query only prunes subtrees.  The
// winner of a step is the candidate of greatest score and, among those, the first in kd order.
//
// rv_kchain is the host restatement, decision for decision (the tree built as the reference builds it, `splitvalue += 1` included): O(m^2 k) checks and
// O(k^2) per gap cost, no range tree.  k_many_kchain is the device form, one job per workgroup of 256 threads, on the records the write pass of
// rv_many_scan.hip has just left in device memory:
//   stage 1  the records (all of n == k: the scan ran with minn = k) -> lengths and points in LDS, 32-bit positions relative to each sequence's begin;
//            the cap by rank over (length, emission index), counted, not sorted
//   stage 2  the order of the targets (rank by dimension 0) and the kd order: ceil(log2(m + 1)) rounds, each ranking the points of a segment by the
//            round's dimension and splitting at n / 2, right half first
//   stage 3  the targets one after another, the threads over the candidates, a reduction over (score, kd order); scores are 64-bit throughout
//   stage 4  backtrack into a reversed path, staged as (record, score) in the room of the job's records
// then the sum of the node counts over the RANKS of the round and k_kchain_write place the paths in CSR arrays.  A job of more than RV_KCHAIN_MEMBERS
// members or RV_KCHAIN_CAP records, or with a coordinate shared by two points, is flagged (RV_KCHAIN_FLAG) and chained from its fetched records: by the
// programme in device memory (rv_kchain_big.hip) or on the host.  rv_kchain is three parts for that: kc_prepare (filter, cap, points, orders -- and why the
// device programme would not take the list), kc_programme_host, kc_backtrack; the device leg shares the first and the last.
#include "../../include/reveal_amd.h"
#include "rv_kchain_big.h"
#include <algorithm>
#include <climits>
#include <vector>

namespace {

constexpr int KTB = 256;
constexpr int KN = RV_KCHAIN_CAP + 1;                 // points: the kept records and p2
constexpr int KP = RV_KCHAIN_MEMBERS + 64;            // coordinates: theirs and p2's
constexpr u32 KNONE = 0xFFFFu;
constexpr u64 KMASK = ((u64)1 << RV_MANY_SCAN_MBITS) - 1;

// ---- host ----
int64_t kc_gapcost_host(const int64_t *a, const int64_t *b, int k, int model, std::vector<int64_t> &D) {
    if (model == 1) {
        int64_t s = 0;
        for (int i = 0; i < k; i++) s += a[i] - b[i];
        return (s < 0 ? -s : s) / k;
    }
    D.resize((size_t)k);
    for (int i = 0; i < k; i++) { const int64_t d = a[i] - b[i]; D[(size_t)i] = d < 0 ? -d : d; }
    if (model == 2) { std::sort(D.begin(), D.end()); return D[(size_t)(k / 2)]; }
    int64_t p = 0;
    for (int i = 0; i < k; i++)
        for (int j = i + 1; j < k; j++) { const int64_t d = D[(size_t)i] - D[(size_t)j]; p += d < 0 ? -d : d; }
    return p;
}

// utils.kdtree + the order range_search pops its leaves in: right subtree first
int kc_kd_order(const std::vector<int64_t> &P, int k, std::vector<int> pts, int depth, std::vector<int> &out) {
    const size_t n = pts.size();
    if (n == 0) return 0;
    if (n == 1) { out.push_back(pts[0]); return 0; }
    if (depth > 8192) { rv_set_error("rv_kchain: identical points (the reference's kdtree does not end on them)"); return -1; }
    const int dim = depth % k;
    std::stable_sort(pts.begin(), pts.end(), [&](int a, int b) { return P[(size_t)a * k + dim] < P[(size_t)b * k + dim]; });
    int64_t split = P[(size_t)pts[n / 2] * k + dim];
    if (split == P[(size_t)pts[0] * k + dim]) split += 1;
    std::vector<int> left, right;
    for (int p : pts) (P[(size_t)p * k + dim] < split ? left : right).push_back(p);
    RV_TRY(kc_kd_order(P, k, std::move(right), depth + 1, out));
    return kc_kd_order(P, k, std::move(left), depth + 1, out);
}

}  // namespace

int kc_prepare(int k, int64_t nrec, const uint32_t *l, const int32_t *n, const int64_t *off, const int64_t *pos, const int64_t *lens, int64_t maxmums,
               int64_t wpen, int64_t wscore, KcPrep &out) {
    out = KcPrep();
    out.k = k;
    std::vector<int64_t> begin((size_t)k);
    int64_t at = 0;
    for (int d = 0; d < k; d++) { if (lens[d] < 0) { rv_set_error("rv_kchain: a negative length"); return -1; } begin[(size_t)d] = at; at += lens[d] + 1; }
    // chain.py:236: the matches in all k sequences, in emission order
    std::vector<int64_t> &kept = out.kept;
    for (int64_t r = 0; r < nrec; r++) if (n[r] == k) {
        if (off[r + 1] - off[r] != k) { rv_set_error("rv_kchain: a match of %d sequences with %lld members", k, (long long)(off[r + 1] - off[r])); return -1; }
        kept.push_back(r);
    }
    // :238-245: stably sorted by length; the cap keeps the last maxmums of that
    std::stable_sort(kept.begin(), kept.end(), [&](int64_t a, int64_t b) { return l[a] < l[b]; });
    if ((int64_t)kept.size() > maxmums && maxmums != 0) kept.erase(kept.begin(), kept.end() - (ptrdiff_t)std::max<int64_t>(maxmums, 0));
    if (kept.size() >= (size_t)INT_MAX / 2) { rv_set_error("rv_kchain: too many records"); return -1; }
    const int m = out.m = (int)kept.size();
    std::vector<int64_t> &P = out.P;
    P.assign((size_t)(m + 1) * k, 0);
    out.L.assign((size_t)m + 1, 0);
    for (int d = 0; d < k; d++) P[(size_t)m * k + d] = lens[d];      // p2
    if (m == 0) return 0;
    // :249-257: a point = the sorted positions, each relative to its sequence's begin
    std::vector<int64_t> tmp((size_t)k);
    for (int i = 0; i < m; i++) {
        for (int q = 0; q < k; q++) tmp[(size_t)q] = pos[off[kept[(size_t)i]] + q];
        std::sort(tmp.begin(), tmp.end());
        for (int d = 0; d < k; d++) P[(size_t)i * k + d] = tmp[(size_t)d] - begin[(size_t)d];
        out.L[(size_t)i] = (int64_t)l[kept[(size_t)i]];
    }
    // :262-266: p2 appended, the list stably sorted by dimension 0, the tree over that list
    std::vector<int> &order = out.order;
    order.resize((size_t)m + 1);
    for (int i = 0; i <= m; i++) order[(size_t)i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return P[(size_t)a * k] < P[(size_t)b * k]; });
    RV_TRY(kc_kd_order(P, k, order, 0, out.kd));
    // what the device programme does not take
    int why = 0;
    if (k > 64) why |= RV_KCHAIN_REFUSE_K;
    if ((int64_t)m > RV_KCHAIN_BIG_CAP || ((int64_t)m + 1) * k > RV_KCHAIN_BIG_MEMBERS) why |= RV_KCHAIN_REFUSE_CAP;
    const int64_t lim = (int64_t)1 << 31;
    int64_t minlen = lens[0];
    __int128 sumlen = 0;
    for (int d = 0; d < k; d++) { if (lens[d] >= lim) why |= RV_KCHAIN_REFUSE_BITS; minlen = std::min(minlen, lens[d]); sumlen += (__int128)lens[d] + 1; }
    for (int i = 0; i < m; i++) {
        const int64_t li = out.L[(size_t)i];
        if (li == 0) why |= RV_KCHAIN_REFUSE_L0;
        if (li >= lim) why |= RV_KCHAIN_REFUSE_BITS;
        for (int d = 0; d < k; d++) { const int64_t p = P[(size_t)i * k + d]; if (p < 0 || p >= lim || p + li > lens[d]) why |= RV_KCHAIN_REFUSE_BITS; }
    }
    std::vector<int64_t> col((size_t)m + 1);
    for (int d = 0; d < k && !(why & RV_KCHAIN_REFUSE_SHARED); d++) {
        for (int i = 0; i <= m; i++) col[(size_t)i] = P[(size_t)i * k + d];
        std::sort(col.begin(), col.end());
        if (std::adjacent_find(col.begin(), col.end()) != col.end()) why |= RV_KCHAIN_REFUSE_SHARED;
    }
    const __int128 pairs = (__int128)k * (k - 1) / 2;
    const __int128 bound = (__int128)(wscore < 0 ? 0 : wscore) * pairs * minlen + (__int128)(wpen < 0 ? 0 : wpen) * pairs * sumlen;      // (rv_kchain.h derives it)
    if (2 * bound >= (__int128)RV_KCHAIN_BIG_SCORE) why |= RV_KCHAIN_REFUSE_SCORE;
    out.refuse = why;
    return 0;
}

int64_t kc_empty_end(const KcPrep &pp, int64_t wpen, int gcmodel) {
    std::vector<int64_t> p1((size_t)pp.k, -1), D;
    return -wpen * kc_gapcost_host(p1.data(), pp.P.data() + (size_t)pp.m * pp.k, pp.k, gcmodel, D);
}

int kc_programme_host(const KcPrep &pp, int64_t wpen, int64_t wscore, int gcmodel, std::vector<int64_t> &score, std::vector<int> &back) {
    const int k = pp.k, m = pp.m;
    const std::vector<int64_t> &P = pp.P, &L = pp.L;
    std::vector<int64_t> p1((size_t)k, -1), D;
    score.assign((size_t)m + 1, 0);
    back.assign((size_t)m + 1, -1);
    std::vector<char> done((size_t)m + 1, 0);
    const int64_t gain = (int64_t)k * (k - 1) / 2;
    for (int t : pp.order) {      // :269-289
        int best = -1;
        int64_t bs = -wpen * kc_gapcost_host(p1.data(), &P[(size_t)t * k], k, gcmodel, D);
        for (int v : pp.kd) {
            if (v == t) continue;
            bool adm = true;
            for (int d = 0; d < k && adm; d++) adm = P[(size_t)v * k + d] <= P[(size_t)t * k + d] && P[(size_t)v * k + d] + L[(size_t)v] <= P[(size_t)t * k + d];
            if (!adm) continue;
            if (!done[(size_t)v] && v != m) { rv_set_error("rv_kchain: a candidate without a score (the reference raises KeyError here)"); return -1; }
            const int64_t sc = score[(size_t)v] + wscore * (L[(size_t)v] * gain) - wpen * kc_gapcost_host(&P[(size_t)v * k], &P[(size_t)t * k], k, gcmodel, D);
            if (sc > bs) { bs = sc; best = v; }
        }
        score[(size_t)t] = bs; back[(size_t)t] = best; done[(size_t)t] = 1;
    }
    return 0;
}

int64_t kc_backtrack(const KcPrep &pp, const std::vector<int64_t> &score, const std::vector<int> &back, uint32_t *out_l, int64_t *out_pos, int64_t *out_score,
                     int64_t *end_score) {
    const int k = pp.k, m = pp.m;
    std::vector<int> path;
    for (int v = back[(size_t)m]; v >= 0; v = back[(size_t)v]) {
        if ((int)path.size() > m || v >= m) { rv_set_error("rv_kchain: broken back-pointer chain"); return -1; }
        path.push_back(v);
    }
    std::reverse(path.begin(), path.end());
    for (size_t x = 0; x < path.size(); x++) {
        out_l[x] = (uint32_t)pp.L[(size_t)path[x]]; out_score[x] = score[(size_t)path[x]];
        for (int d = 0; d < k; d++) out_pos[x * (size_t)k + d] = pp.P[(size_t)path[x] * k + d];
    }
    *end_score = score[(size_t)m];
    return (int64_t)path.size();
}

extern "C" int64_t rv_kchain(int k, int64_t nrec, const uint32_t *l, const int32_t *n, const int64_t *off, const uint16_t *so, const int64_t *pos,
                             const int64_t *lens, int64_t maxmums, int64_t wpen, int64_t wscore, int gcmodel, uint32_t *out_l, int64_t *out_pos,
                             int64_t *out_score, int64_t *end_score) {
    if (k < 2 || nrec < 0 || !lens || !end_score || gcmodel < 0 || gcmodel > 2 || (nrec > 0 && (!l || !n || !off || !so || !pos || !out_l || !out_pos || !out_score))) {
        rv_set_error("rv_kchain: bad arguments");
        return -1;
    }
    try {
        KcPrep pp;
        RV_TRY(kc_prepare(k, nrec, l, n, off, pos, lens, maxmums, wpen, wscore, pp));
        if (pp.m == 0) { *end_score = kc_empty_end(pp, wpen, gcmodel); return 0; }      // (chain() returns [p1, p2] and scores nothing)
        std::vector<int64_t> score;
        std::vector<int> back;
        RV_TRY(kc_programme_host(pp, wpen, wscore, gcmodel, score, back));
        return kc_backtrack(pp, score, back, out_l, out_pos, out_score, end_score);
    } catch (const std::exception &e) { rv_set_error("rv_kchain: %s", e.what()); return -1; }
}

// why the device programme would leave this list to the host (RV_KCHAIN_REFUSE_* of rv_kchain.h; 0: it takes it); host only, no device is asked for
extern "C" int rv_kchain_admit(int k, int64_t nrec, const uint32_t *l, const int32_t *n, const int64_t *off, const int64_t *pos, const int64_t *lens,
                               int64_t maxmums, int64_t wpen, int64_t wscore) {
    if (k < 2 || nrec < 0 || !lens || (nrec > 0 && (!l || !n || !off || !pos))) { rv_set_error("rv_kchain_admit: bad arguments"); return -1; }
    try {
        KcPrep pp;
        RV_TRY(kc_prepare(k, nrec, l, n, off, pos, lens, maxmums, wpen, wscore, pp));
        return pp.refuse;
    } catch (const std::exception &e) { rv_set_error("rv_kchain_admit: %s", e.what()); return -1; }
}

// ---- device ----
namespace {

struct KcShared {
    u32 P[KP];                    // point i: P[i k .. i k + k); point m = p2
    u32 L[KN];
    uint16_t ord0[KN];            // targets in processing order; after the programme: the reversed path
    uint16_t kdr[KN];             // kd order of a point
    uint16_t orig[KN];            // its record, counted from the job's first
    u32 loc[64], len[64];
    union {
        struct { u32 L[KN]; uint16_t idx[KN]; } s1;                            // records in emission order, their place after the cap
        struct { uint16_t perm[2][KN], segS[2][KN], segN[2][KN]; } s2;          // the kd rounds, double-buffered
        struct { int64_t score[KN]; uint16_t back[KN]; } s3;
    } u;
    int64_t rs[KTB / 64];
    u32 rk[KTB / 64];
    int cnt;
};

__global__ __launch_bounds__(KTB) void k_many_kchain(RvManyScanRound R, RvKchainRound K, RvKchainArgs A) {
    __shared__ KcShared S;
    const int j = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (j >= R.njobs) return;
    const int64_t j0 = R.off[j], j1 = R.off[j + 1];
    const int s0 = R.sfirst[j];
    const int k = R.sfirst[j + 1] - s0;
    const u64 r0 = K.first[j] >> RV_MANY_SCAN_MBITS, r1 = K.first[j + 1] >> RV_MANY_SCAN_MBITS, m0 = K.first[j] & KMASK, m1 = K.first[j + 1] & KMASK;
    if (tid == 0) { K.flag[j] = 0; K.end[j] = 0; }
    if (!(j0 >= 0 && j0 < j1 && j1 <= R.m && s0 >= 0 && k >= 2 && k <= 64 && s0 + k <= R.nbeg && r0 <= r1 && r1 <= K.nrec && m0 <= m1 && m1 <= K.nmem)) {
        if (tid == 0) atomicOr(K.err, 1u);
        return;
    }
    const u64 c64 = r1 - r0;
    if (c64 * (u64)k > RV_KCHAIN_MEMBERS || c64 > (u64)(A.cap < RV_KCHAIN_CAP ? A.cap : RV_KCHAIN_CAP) || m1 - m0 != c64 * (u64)k) {      // (uniform: the host's job)
        if (tid == 0) K.flag[j] = RV_KCHAIN_FLAG;
        return;
    }
    const int c = (int)c64;
    int bad = 0;
    if (tid < k) {
        const int64_t lo = R.loc[s0 + tid], nx = tid + 1 < k ? (int64_t)R.loc[s0 + tid + 1] : j1 - j0;
        if (lo < 0 || nx - lo - 1 < 0 || nx > j1 - j0) bad = 1;
        S.loc[tid] = (u32)lo; S.len[tid] = (u32)(nx - lo - 1);
    }
    if (__syncthreads_or(bad)) { if (tid == 0) atomicOr(K.err, 1u); return; }
    // stage 1: the records (coalesced over records), the cap, the points (coalesced over members)
    for (int i = tid; i < c; i += KTB) {
        const RvManyScanRec r = K.rec[r0 + (u64)i];
        if (r.n != (u32)k || r.moff != m0 + (u64)i * (u64)k || r.l == 0) bad = 1;
        S.u.s1.L[i] = r.l;
    }
    if (__syncthreads_or(bad)) { if (tid == 0) K.flag[j] = RV_KCHAIN_FLAG; return; }      // (a record of fewer sequences: the host filters)
    int m = c;
    if (A.maxmums != 0 && (int64_t)c > A.maxmums) {
        m = (int)(A.maxmums > 0 ? A.maxmums : 0);
        const int drop = c - m;
        for (int i = tid; i < c; i += KTB) {
            const u32 li = S.u.s1.L[i];
            int rank = 0;
            for (int x = 0; x < c; x++) { const u32 lx = S.u.s1.L[x]; rank += (lx < li || (lx == li && x < i)) ? 1 : 0; }
            S.u.s1.idx[i] = (uint16_t)(rank >= drop ? rank - drop : KNONE);
        }
    } else for (int i = tid; i < c; i += KTB) S.u.s1.idx[i] = (uint16_t)i;
    for (int x = tid; x < (m + 1) * k; x += KTB) S.P[x] = 0xFFFFFFFFu;
    __syncthreads();
    for (int i = tid; i < c; i += KTB) { const u32 ni = S.u.s1.idx[i]; if (ni != KNONE) { S.L[ni] = S.u.s1.L[i]; S.orig[ni] = (uint16_t)i; } }
    for (int x = tid; x < c * k; x += KTB) {
        const int i = x / k;
        const u32 ni = S.u.s1.idx[i];
        if (ni == KNONE) continue;
        const u32 s = K.so[m0 + (u64)x];
        if (s >= (u32)k) { bad = 1; continue; }
        const int64_t rel = (int64_t)K.pos[m0 + (u64)x] - (int64_t)S.loc[s];
        if (rel < 0 || rel + (int64_t)S.u.s1.L[i] > (int64_t)S.len[s]) { bad = 1; continue; }
        S.P[ni * k + s] = (u32)rel;
    }
    if (tid < k) S.P[m * k + tid] = S.len[tid];
    if (tid == 0) S.L[m] = 0;
    __syncthreads();
    for (int x = tid; x < m * k; x += KTB) if (S.P[x] == 0xFFFFFFFFu) bad = 1;      // (two members in one sequence)
    if (__syncthreads_or(bad)) { if (tid == 0) atomicOr(K.err, 2u); return; }
    // stage 2: the order of the targets, then the kd order
    const int n1 = m + 1;
    int dup = 0;
    for (int i = tid; i < n1; i += KTB) {
        const u32 pi = S.P[i * k];
        int r = 0;
        for (int x = 0; x < n1; x++) { const u32 q = S.P[x * k]; r += (q < pi || (q == pi && x < i)) ? 1 : 0; dup |= (q == pi && x != i) ? 1 : 0; }
        S.ord0[r] = (uint16_t)i;
        S.u.s2.perm[0][i] = (uint16_t)i; S.u.s2.segS[0][i] = 0; S.u.s2.segN[0][i] = (uint16_t)n1;
    }
    __syncthreads();
    int cur = 0;
    for (int big = n1, depth = 0; big > 1; big -= big / 2, depth++) {
        const int dim = depth % k;
        for (int x = tid; x < n1; x += KTB) {
            const int s = S.u.s2.segS[cur][x], n = S.u.s2.segN[cur][x], i = S.u.s2.perm[cur][x];
            int nx = x, ns = s, nn = n;
            if (n > 1) {
                const u32 pi = S.P[i * k + dim];
                int r = 0;
                for (int y = s; y < s + n; y++) {
                    const int i2 = S.u.s2.perm[cur][y];
                    const u32 q = S.P[i2 * k + dim];
                    r += (q < pi || (q == pi && i2 < i)) ? 1 : 0; dup |= (q == pi && i2 != i) ? 1 : 0;
                }
                const int nl = n / 2, nr = n - nl;      // (the first n / 2 go left; the right half comes first in the order)
                if (r >= nl) { nx = s + (r - nl); nn = nr; } else { nx = s + nr + r; ns = s + nr; nn = nl; }
            }
            S.u.s2.perm[cur ^ 1][nx] = (uint16_t)i; S.u.s2.segS[cur ^ 1][nx] = (uint16_t)ns; S.u.s2.segN[cur ^ 1][nx] = (uint16_t)nn;
        }
        __syncthreads();
        cur ^= 1;
    }
    for (int x = tid; x < n1; x += KTB) S.kdr[S.u.s2.perm[cur][x]] = (uint16_t)x;
    if (__syncthreads_or(dup)) { if (tid == 0) K.flag[j] = RV_KCHAIN_FLAG; return; }      // (a shared coordinate: the reference's tree takes its `splitvalue += 1` turn)
    // stage 3: the dynamic programme
    const int64_t gain = (int64_t)(k * (k - 1) / 2);
    for (int ti = 0; ti < n1; ti++) {
        const int t = S.ord0[ti];
        const u32 *pt = &S.P[t * k];
        int64_t bs = INT64_MIN;
        u32 bk = 0xFFFFFFFFu;
        for (int v = tid; v < m; v += KTB) {
            if (v == t) continue;
            const u32 lv = S.L[v];
            const u32 *pv = &S.P[v * k];
            bool adm = true;
            for (int d = 0; d < k; d++) if (pv[d] + lv > pt[d]) { adm = false; break; }
            if (!adm) continue;      // (admissible: in front of t in dimension 0, so it has its score)
            const int64_t sc = S.u.s3.score[v] + A.wscore * ((int64_t)lv * gain) - A.wpen * kc_gap(KcStrided{pv, 1}, KcStrided{pt, 1}, k, A.gcmodel);
            const u32 key = (u32)S.kdr[v] << 16 | (u32)v;
            if (sc > bs || (sc == bs && key < bk)) { bs = sc; bk = key; }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const int64_t os = __shfl_xor(bs, o);
            const u32 ok = __shfl_xor(bk, o);
            if (os > bs || (os == bs && ok < bk)) { bs = os; bk = ok; }
        }
        if ((tid & 63) == 0) { S.rs[tid >> 6] = bs; S.rk[tid >> 6] = bk; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < KTB / 64; w++) if (S.rs[w] > bs || (S.rs[w] == bs && S.rk[w] < bk)) { bs = S.rs[w]; bk = S.rk[w]; }
            const int64_t ps = -A.wpen * kc_gap(KcP1(), KcStrided{pt, 1}, k, A.gcmodel);
            const bool take = bk != 0xFFFFFFFFu && bs > ps;      // strict: p1 stays where nothing beats it
            S.u.s3.score[t] = take ? bs : ps;
            S.u.s3.back[t] = (uint16_t)(take ? (bk & 0xFFFFu) : KNONE);
        }
        __syncthreads();
    }
    // stage 4: backtrack
    if (tid == 0) {
        int cnt = 0;
        u32 v = S.u.s3.back[m];
        while (v != KNONE && cnt <= m) { if (v >= (u32)m) { cnt = m + 1; break; } S.ord0[cnt++] = (uint16_t)v; v = S.u.s3.back[v]; }
        if (cnt > m) { atomicOr(K.err, 4u); cnt = 0; }      // (a back-pointer that leaves the job, or a cycle)
        S.cnt = cnt;
    }
    __syncthreads();
    const int cnt = S.cnt;
    for (int x = tid; x < cnt; x += KTB) {
        const int v = S.ord0[cnt - 1 - x];
        K.stage_rec[r0 + (u64)x] = (u32)(r0 + (u64)S.orig[v]);
        K.stage_score[r0 + (u64)x] = S.u.s3.score[v];
    }
    if (tid == 0) { K.nodes[j0] = (u64)cnt << RV_MANY_SCAN_MBITS | (u64)cnt * (u64)k; K.end[j] = S.u.s3.score[m]; }
}

__global__ __launch_bounds__(KTB) void k_kchain_first(const u64 *__restrict__ nodes, const int64_t *__restrict__ off, int njobs, int64_t m, u64 *__restrict__ cfirst,
                                                      u32 *__restrict__ err) {
    const int j = (int)(blockIdx.x * KTB + threadIdx.x);
    if (j > njobs) return;
    const int64_t o = off[j];
    const bool ok = o >= 0 && o <= m && (j < njobs || o == m) && (j == 0 ? o == 0 : off[j - 1] < o);
    if (!ok) atomicOr(err, 1u);
    cfirst[j] = ok ? nodes[o] : 0;
}

// a thread per staged slot: the slot's job by the scan's sums, then the node at the place the chain's sums give it
__global__ __launch_bounds__(KTB) void k_kchain_write(RvManyScanRound R, RvKchainRound K, const u64 *__restrict__ cfirst, u32 *__restrict__ out_l,
                                                      int64_t *__restrict__ out_score, u32 *__restrict__ out_pos, u64 nnodes, u64 nmem) {
    const u64 x = (u64)blockIdx.x * KTB + threadIdx.x;
    if (x >= K.nrec) return;
    int lo = 0, hi = R.njobs;      // the last job whose records begin at or in front of x
    while (lo < hi) { const int mid = (lo + hi) >> 1; if ((K.first[mid] >> RV_MANY_SCAN_MBITS) <= x) lo = mid + 1; else hi = mid; }
    const int j = lo - 1;
    if (j < 0) { atomicOr(K.err, 1u); return; }
    const u64 r0 = K.first[j] >> RV_MANY_SCAN_MBITS, r1 = K.first[j + 1] >> RV_MANY_SCAN_MBITS;
    const u64 idx = x - r0, n0 = cfirst[j] >> RV_MANY_SCAN_MBITS, nn = (cfirst[j + 1] >> RV_MANY_SCAN_MBITS) - n0;
    if (x >= r1 || idx >= nn) return;
    const int s0 = R.sfirst[j];
    const int k = R.sfirst[j + 1] - s0;
    const u64 o = n0 + idx, mo = (cfirst[j] & KMASK) + idx * (u64)k;
    const u32 rr = K.stage_rec[x];
    if (k < 2 || k > 64 || s0 < 0 || s0 + k > R.nbeg || o >= nnodes || mo + (u64)k > nmem || rr < r0 || rr >= r1) { atomicOr(K.err, 4u); return; }
    const RvManyScanRec r = K.rec[rr];
    if (r.n != (u32)k || r.moff + (u64)k > K.nmem) { atomicOr(K.err, 4u); return; }
    out_l[o] = r.l; out_score[o] = K.stage_score[x];
    for (int q = 0; q < k; q++) {
        const u32 s = K.so[r.moff + (u64)q];
        if (s >= (u32)k) { atomicOr(K.err, 2u); return; }
        out_pos[mo + s] = K.pos[r.moff + (u64)q] - (u32)R.loc[s0 + (int)s];
    }
}

}  // namespace

int rv_many_kchain_run(Workspace &ws, const RvManyScanRound &R, const RvKchainRound &K, const RvKchainArgs &A, int64_t *launches) {
    if (R.njobs < 1) { rv_set_error("rv_many_kchain: a round of %d jobs", R.njobs); return -1; }
    hipLaunchKernelGGL(k_many_kchain, dim3((unsigned)R.njobs), dim3(KTB), 0, ws.stream, R, K, A);
    RV_LAUNCH_CHECK();
    if (launches) *launches += 1;
    return 0;
}

int rv_many_kchain_first(Workspace &ws, const RvManyScanRound &R, const RvKchainRound &K, u64 *cfirst, int64_t *launches) {
    hipLaunchKernelGGL(k_kchain_first, dim3((unsigned)ceil_div((int64_t)R.njobs + 1, KTB)), dim3(KTB), 0, ws.stream, K.nodes, R.off, R.njobs, R.m, cfirst, K.err);
    RV_LAUNCH_CHECK();
    if (launches) *launches += 1;
    return 0;
}

int rv_many_kchain_write(Workspace &ws, const RvManyScanRound &R, const RvKchainRound &K, const u64 *cfirst, u32 *out_l, int64_t *out_score, u32 *out_pos,
                         u64 nnodes, u64 nmem, int64_t *launches) {
    if (!nnodes || !K.nrec) return 0;
    hipLaunchKernelGGL(k_kchain_write, dim3((unsigned)ceil_div((int64_t)K.nrec, KTB)), dim3(KTB), 0, ws.stream, R, K, cfirst, out_l, out_score, out_pos, nnodes, nmem);
    RV_LAUNCH_CHECK();
    if (launches) *launches += 1;
    return 0;
}
