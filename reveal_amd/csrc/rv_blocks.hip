// rv_blocks.hip -- the first stage of `reveal transform` (transform.py:252-293) behind getblocks: addctginfo + clustermumsbydiagonal.
//
// The rule (one statement, both programmes below follow it).  A record is (l, a, b), b in forward coordinates.  end[i] = the '$' of the i-th
// sequence.  refid = #{i: end[i] < a}, ctgid = #{i: end[i] < b}.  cluster = 0: one block per record, ascending (b, a).  cluster = 1: the
// records in the order of (first, a), first = a - b for o = 0 and a + b + l for o = 1 -- the reference sorts by (a - b, a + b) resp.
// (a + b + l, a - (b + l)), and on one value of `first` both second components grow with a, so this is the same total order --; record i
// continues the cluster of record i-1 iff it has the same `first`, the same two ids, and a_i - (a_{i-1} + l_{i-1}) < maxdist; a negative
// distance there is an error.  A cluster with first member F and last member L is the block (a_F, a_L + l_L, b_F, b_L + l_L) for o = 0 and
// (a_F, a_L + l_L, b_L, b_F + l_F) for o = 1, its score the sum of l; blocks below minclustsize are dropped, the order stays.
//
// Device programme: k_blk_keys (record -> ids, key, record number) -> rv_radix_sort_pairs -> k_blk_heads (a position and its predecessor)
// -> rv_exclusive_sum_u32 of the heads (cluster numbers) and rv_exclusive_sum_u64 of l (scores as differences) -> k_blk_starts ->
// k_blk_emit (one thread per cluster: its first and its last record) -> rv_exclusive_sum_u32 of the keep flags -> k_blk_compact.
// Nothing walks the members of a cluster, nothing is ordered by an atomic, and the launches depend on the key width only.
// The key: (first << abits) | a where first and a fit 64 bits together (every index of the 32-bit library, and of the 64-bit one while
// bits(2 n) + bits(nsep0) <= 64); otherwise two stable sorts, by a and then by first.
#include "rv_blocks.h"
#include <algorithm>
#include <numeric>

namespace {

struct BlkDev {
    int64_t *A, *B; u32 *L; int32_t *RID, *CID;
    const int64_t *end; int64_t nseq;
    int o, cluster; int64_t bias;
    u32 n;
};

__device__ __forceinline__ u64 blk_first(const BlkDev &d, int64_t a, int64_t b, u32 l) {
    if (!d.cluster) return (u64)b;
    return d.o ? (u64)(a + b + (int64_t)l) : (u64)(a - b + d.bias);
}
// #{i: end[i] < x}
__device__ __forceinline__ int32_t blk_seq(const int64_t *__restrict__ end, int64_t nseq, int64_t x) {
    int64_t lo = 0, hi = nseq;
    while (lo < hi) { const int64_t mid = lo + ((hi - lo) >> 1); if (end[mid] < x) lo = mid + 1; else hi = mid; }
    return (int32_t)lo;
}

// mode 0: the one-sort key (first << abits) | a;  mode 1: a (the first of two stable sorts);  mode 2: first of the record at sorted position i
// (perm from the first sort).  Modes 0 and 1 also bring the records into A / B / L (from the scan's list, with the rc map of b) and look the ids up.
__global__ __launch_bounds__(256) void k_blk_keys(BlkDev d, const RvPairRec *__restrict__ recs, int rc_map, int64_t nsep0, int64_t nT, int mode, int abits,
                                                   const u32 *__restrict__ perm, u64 *__restrict__ keys, u32 *__restrict__ vals) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= d.n) return;
    if (mode == 2) {
        const u32 r = perm[i];
        keys[i] = blk_first(d, d.A[r], d.B[r], d.L[r]);
        vals[i] = r;
        return;
    }
    int64_t a, b; u32 l;
    if (recs) {
        const RvPairRec r = recs[i];
        a = (int64_t)r.a; b = (int64_t)r.b; l = r.l;
        if (rc_map) b = nsep0 + (nT - b - (int64_t)l);
        d.A[i] = a; d.B[i] = b; d.L[i] = l;
    } else {
        a = d.A[i]; b = d.B[i]; l = d.L[i];
    }
    d.RID[i] = blk_seq(d.end, d.nseq, a);
    d.CID[i] = blk_seq(d.end, d.nseq, b);
    keys[i] = mode == 0 ? ((blk_first(d, a, b, l) << abits) | (u64)a) : (u64)a;
    vals[i] = i;
}

// head[i] = 1 where sorted position i starts a cluster; l64[i] = its length; both arrays get a zero at [n] for the sums
__global__ __launch_bounds__(256) void k_blk_heads(BlkDev d, const u32 *__restrict__ perm, int64_t maxdist, u32 *__restrict__ head, u64 *__restrict__ l64, u32 *__restrict__ hdr) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= d.n) return;
    const u32 r = perm[i];
    const int64_t a = d.A[r];
    const u32 l = d.L[r];
    u32 h = 1;
    if (d.cluster && i > 0) {
        const u32 p = perm[i - 1];
        const int64_t ap = d.A[p]; const u32 lp = d.L[p];
        if (blk_first(d, a, d.B[r], l) == blk_first(d, ap, d.B[p], lp) && d.RID[r] == d.RID[p] && d.CID[r] == d.CID[p]) {
            const int64_t dist = a - (ap + (int64_t)lp);
            if (dist < 0) atomicOr(&hdr[2], 1u);
            if (dist < maxdist) h = 0;
        }
    }
    head[i] = h; l64[i] = (u64)l;
    if (i == 0) { head[d.n] = 0; l64[d.n] = 0; }
}

// cnum = exclusive sum of head over n + 1 entries: start[c] = sorted position of the first member of cluster c, start[number of clusters] = n
__global__ __launch_bounds__(256) void k_blk_starts(u32 n, const u32 *__restrict__ cnum, u32 *__restrict__ start) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const u32 c = cnum[i];
    if (cnum[i + 1] != c) start[c] = i;
    if (i == n - 1) start[cnum[n]] = n;
}

// SoA of n blocks: five int64 arrays of n, then two int32 arrays of n
struct BlkSoA {
    int64_t *s1, *e1, *s2, *e2, *score; int32_t *refid, *ctgid;
    __host__ __device__ BlkSoA(void *p, size_t n) {
        s1 = (int64_t *)p; e1 = s1 + n; s2 = e1 + n; e2 = s2 + n; score = e2 + n;
        refid = (int32_t *)(score + n); ctgid = refid + n;
    }
};

__global__ __launch_bounds__(256) void k_blk_emit(BlkDev d, const u32 *__restrict__ perm, const u32 *__restrict__ cnum, const u32 *__restrict__ start, const u64 *__restrict__ lsum,
                                                   int64_t minclustsize, void *tmp, u32 *__restrict__ keep) {
    const u32 c = blockIdx.x * 256u + threadIdx.x;
    if (c >= d.n) return;
    if (c == 0) keep[d.n] = 0;
    if (c >= cnum[d.n]) { keep[c] = 0; return; }
    const u32 f = start[c], e = start[c + 1] - 1u;
    const u32 F = perm[f], Lr = perm[e];
    const int64_t score = (int64_t)(lsum[e + 1] - lsum[f]);
    BlkSoA t(tmp, d.n);
    t.s1[c] = d.A[F]; t.e1[c] = d.A[Lr] + (int64_t)d.L[Lr];
    if (d.o) { t.s2[c] = d.B[Lr]; t.e2[c] = d.B[F] + (int64_t)d.L[F]; }
    else { t.s2[c] = d.B[F]; t.e2[c] = d.B[Lr] + (int64_t)d.L[Lr]; }
    t.score[c] = score; t.refid[c] = d.RID[F]; t.ctgid[c] = d.CID[F];
    keep[c] = (!d.cluster || score >= minclustsize) ? 1u : 0u;
}

// koff = exclusive sum of keep over n + 1 entries; hdr = {clusters, kept blocks, error bits (k_blk_heads), 0}
__global__ __launch_bounds__(256) void k_blk_compact(u32 n, const u32 *__restrict__ cnum, const u32 *__restrict__ koff, const void *tmp, void *out, u32 *__restrict__ hdr) {
    const u32 c = blockIdx.x * 256u + threadIdx.x;
    if (c >= n) return;
    if (c == 0) { hdr[0] = cnum[n]; hdr[1] = koff[n]; }
    const u32 k = koff[c];
    if (koff[c + 1] == k) return;
    const BlkSoA t(const_cast<void *>(tmp), n); BlkSoA w(out, n);
    w.s1[k] = t.s1[c]; w.e1[k] = t.e1[c]; w.s2[k] = t.s2[c]; w.e2[k] = t.e2[c]; w.score[k] = t.score[c]; w.refid[k] = t.refid[c]; w.ctgid[k] = t.ctgid[c];
}

int bits_of(u64 v) { int b = 0; while (v) { b++; v >>= 1; } return b ? b : 1; }

}  // namespace

int rv_blocks_device(Workspace &ws, const RvBlkIn &in, const int64_t *end, int64_t nseq, const RvBlkArgs &args, RvBlkOut &out) {
    out.clear();
    const int64_t n64 = in.n;
    if (n64 < 0 || nseq < 0 || (nseq && !end)) { rv_set_error("blocks: bad arguments"); return -1; }
    out.nmums = n64;
    if (n64 == 0) return 0;
    if (n64 > 0xfffffff0ll) { rv_set_error("blocks: more than 2^32 - 16 records"); return -1; }
    const int64_t lim = (int64_t)1 << 61;
    if (in.max_a < 0 || in.max_b < 0 || in.max_l < 0 || in.max_a >= lim || in.max_b >= lim || in.max_l >= lim) { rv_set_error("blocks: coordinates outside 0 .. 2^61"); return -1; }
    const u32 n = (u32)n64;
    const size_t N = (size_t)n, N1 = N + 1;
    hipStream_t q = ws.stream;
    DBuf *B = ws.blk;
    RV_TRY(B[0].reserve(N * 8)); RV_TRY(B[1].reserve(N * 8)); RV_TRY(B[2].reserve(N * 4)); RV_TRY(B[3].reserve(N * 4)); RV_TRY(B[4].reserve(N * 4));
    RV_TRY(B[5].reserve(N1 * 8)); RV_TRY(B[6].reserve(N1 * 8)); RV_TRY(B[7].reserve(N1 * 4)); RV_TRY(B[8].reserve(N1 * 4)); RV_TRY(B[9].reserve(N1 * 4));
    RV_TRY(B[10].reserve((size_t)std::max<int64_t>(nseq, 1) * 8)); RV_TRY(B[11].reserve(N * 48)); RV_TRY(B[12].reserve(N * 48)); RV_TRY(B[13].reserve(N1 * 4));
    RV_TRY(B[14].reserve(64));
    BlkDev d;
    d.A = B[0].as<int64_t>(); d.B = B[1].as<int64_t>(); d.L = B[2].as<u32>(); d.RID = B[3].as<int32_t>(); d.CID = B[4].as<int32_t>();
    d.end = B[10].as<int64_t>(); d.nseq = nseq; d.o = args.o ? 1 : 0; d.cluster = args.cluster ? 1 : 0; d.bias = in.max_b; d.n = n;
    u32 *hdr = B[14].as<u32>();
    RV_HIP(hipMemsetAsync(hdr, 0, 16, q));
    if (nseq) RV_HIP(hipMemcpyAsync(B[10].p, end, (size_t)nseq * 8, hipMemcpyHostToDevice, q));
    if (!in.recs) {
        if (!in.l || !in.a || !in.b) { rv_set_error("blocks: null record arrays"); return -1; }
        RV_HIP(hipMemcpyAsync(d.A, in.a, N * 8, hipMemcpyHostToDevice, q));
        RV_HIP(hipMemcpyAsync(d.B, in.b, N * 8, hipMemcpyHostToDevice, q));
        RV_HIP(hipMemcpyAsync(d.L, in.l, N * 4, hipMemcpyHostToDevice, q));
    }
    RV_HIP(hipStreamSynchronize(q));      // (the host arrays are the caller's)
    const u64 max_first = !d.cluster ? (u64)in.max_b : (u64)in.max_a + (u64)in.max_b + (d.o ? (u64)in.max_l : 0ull);
    const int fbits = bits_of(max_first), abits = bits_of((u64)in.max_a);
    const unsigned grid = (unsigned)ceil_div(n64, 256);
    u64 *ka = B[5].as<u64>(), *kb = B[6].as<u64>();
    u32 *va = B[7].as<u32>(), *vb = B[8].as<u32>();
    int f = 0;
    if (fbits + abits <= 64) {
        hipLaunchKernelGGL(k_blk_keys, dim3(grid), dim3(256), 0, q, d, in.recs, in.rc_map, in.nsep0, in.nT, 0, abits, (const u32 *)nullptr, ka, va);
        RV_LAUNCH_CHECK();
        RV_TRY(rv_radix_sort_pairs<u32>(ws, ka, va, kb, vb, n64, 0, fbits + abits, &f));
        if (f) { std::swap(ka, kb); std::swap(va, vb); }
    } else {
        hipLaunchKernelGGL(k_blk_keys, dim3(grid), dim3(256), 0, q, d, in.recs, in.rc_map, in.nsep0, in.nT, 1, 0, (const u32 *)nullptr, ka, va);
        RV_LAUNCH_CHECK();
        RV_TRY(rv_radix_sort_pairs<u32>(ws, ka, va, kb, vb, n64, 0, abits, &f));
        if (f) { std::swap(ka, kb); std::swap(va, vb); }
        hipLaunchKernelGGL(k_blk_keys, dim3(grid), dim3(256), 0, q, d, (const RvPairRec *)nullptr, 0, (int64_t)0, (int64_t)0, 2, 0, (const u32 *)va, kb, vb);
        RV_LAUNCH_CHECK();
        RV_TRY(rv_radix_sort_pairs<u32>(ws, kb, vb, ka, va, n64, 0, fbits, &f));
        if (!f) { std::swap(ka, kb); std::swap(va, vb); }
    }
    // sorted: record numbers in va; the keys are not read again -- ka takes the lengths and their sums, vb the heads and the cluster numbers
    const u32 *perm = va;
    u32 *cnum = vb; u64 *lsum = ka;
    u32 *start = B[9].as<u32>(), *keep = B[13].as<u32>();
    hipLaunchKernelGGL(k_blk_heads, dim3(grid), dim3(256), 0, q, d, perm, args.maxdist, cnum, lsum, hdr);
    RV_LAUNCH_CHECK();
    RV_TRY(rv_exclusive_sum_u32(ws, cnum, cnum, n64 + 1));
    RV_TRY(rv_exclusive_sum_u64(ws, lsum, lsum, n64 + 1));
    hipLaunchKernelGGL(k_blk_starts, dim3(grid), dim3(256), 0, q, n, (const u32 *)cnum, start);
    RV_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_blk_emit, dim3(grid), dim3(256), 0, q, d, perm, (const u32 *)cnum, (const u32 *)start, (const u64 *)lsum, args.minclustsize, B[11].p, keep);
    RV_LAUNCH_CHECK();
    RV_TRY(rv_exclusive_sum_u32(ws, keep, keep, n64 + 1));
    hipLaunchKernelGGL(k_blk_compact, dim3(grid), dim3(256), 0, q, n, (const u32 *)cnum, (const u32 *)keep, (const void *)B[11].p, B[12].p, hdr);
    RV_LAUNCH_CHECK();
    u32 hh[4] = {0, 0, 0, 0};
    RV_TRY(rv_read_back(ws, hh, hdr, 16));
    if (hh[2]) { rv_set_error("blocks: overlapping matches on a diagonal"); return -1; }
    if (hh[0] > n || hh[1] > hh[0]) { rv_set_error("blocks: inconsistent counts from the device"); return -1; }
    out.nclusters = hh[0];
    const size_t k = hh[1];
    out.s1.resize(k); out.e1.resize(k); out.s2.resize(k); out.e2.resize(k); out.score.resize(k); out.refid.resize(k); out.ctgid.resize(k);
    if (k) {
        const BlkSoA w(B[12].p, N);
        RV_HIP(hipMemcpyAsync(out.s1.data(), w.s1, k * 8, hipMemcpyDeviceToHost, q));
        RV_HIP(hipMemcpyAsync(out.e1.data(), w.e1, k * 8, hipMemcpyDeviceToHost, q));
        RV_HIP(hipMemcpyAsync(out.s2.data(), w.s2, k * 8, hipMemcpyDeviceToHost, q));
        RV_HIP(hipMemcpyAsync(out.e2.data(), w.e2, k * 8, hipMemcpyDeviceToHost, q));
        RV_HIP(hipMemcpyAsync(out.score.data(), w.score, k * 8, hipMemcpyDeviceToHost, q));
        RV_HIP(hipMemcpyAsync(out.refid.data(), w.refid, k * 4, hipMemcpyDeviceToHost, q));
        RV_HIP(hipMemcpyAsync(out.ctgid.data(), w.ctgid, k * 4, hipMemcpyDeviceToHost, q));
        RV_HIP(hipStreamSynchronize(q));
    }
    return 0;
}

// ---- the host programme: the same rule, std::stable_sort and one walk --------------------------------------------------------------------------------
int rv_blocks_rule_host(int64_t n, const uint32_t *l, const int64_t *a, const int64_t *b, const int64_t *end, int64_t nseq, const RvBlkArgs &args, RvBlkOut &out) {
    out.clear();
    if (n < 0 || nseq < 0 || (n && (!l || !a || !b)) || (nseq && !end)) { rv_set_error("blocks: bad arguments"); return -1; }
    out.nmums = n;
    if (n == 0) return 0;
    try {
        const int o = args.o ? 1 : 0;
        std::vector<int64_t> ord((size_t)n);
        std::iota(ord.begin(), ord.end(), (int64_t)0);
        std::vector<int32_t> rid((size_t)n), cid((size_t)n);
        for (int64_t i = 0; i < n; i++) {
            if (a[i] < 0 || b[i] < 0 || a[i] >= ((int64_t)1 << 61) || b[i] >= ((int64_t)1 << 61)) { rv_set_error("blocks: coordinates outside 0 .. 2^61"); return -1; }
            rid[(size_t)i] = (int32_t)(std::lower_bound(end, end + nseq, a[i]) - end);
            cid[(size_t)i] = (int32_t)(std::lower_bound(end, end + nseq, b[i]) - end);
        }
        auto first = [&](int64_t i) -> int64_t { return !args.cluster ? b[i] : o ? a[i] + b[i] + (int64_t)l[i] : a[i] - b[i]; };
        std::stable_sort(ord.begin(), ord.end(), [&](int64_t x, int64_t y) { const int64_t fx = first(x), fy = first(y); return fx != fy ? fx < fy : a[x] < a[y]; });
        auto push = [&](int64_t F, int64_t L, int64_t score) {
            out.nclusters++;
            if (args.cluster && score < args.minclustsize) return;
            out.s1.push_back(a[F]); out.e1.push_back(a[L] + (int64_t)l[L]);
            if (o) { out.s2.push_back(b[L]); out.e2.push_back(b[F] + (int64_t)l[F]); }
            else { out.s2.push_back(b[F]); out.e2.push_back(b[L] + (int64_t)l[L]); }
            out.score.push_back(score); out.refid.push_back(rid[(size_t)F]); out.ctgid.push_back(cid[(size_t)F]);
        };
        int64_t F = ord[0], score = l[ord[0]];
        for (int64_t i = 1; i < n; i++) {
            const int64_t r = ord[(size_t)i], p = ord[(size_t)i - 1];
            bool cont = false;
            if (args.cluster && first(r) == first(p) && rid[(size_t)r] == rid[(size_t)p] && cid[(size_t)r] == cid[(size_t)p]) {
                const int64_t dist = a[r] - (a[p] + (int64_t)l[p]);
                if (dist < 0) { rv_set_error("blocks: overlapping matches on a diagonal"); return -1; }
                cont = dist < args.maxdist;
            }
            if (cont) { score += l[r]; continue; }
            push(F, p, score);
            F = r; score = l[r];
        }
        push(F, ord[(size_t)n - 1], score);
    } catch (...) { rv_set_error("blocks: out of host memory"); return -1; }
    return 0;
}
