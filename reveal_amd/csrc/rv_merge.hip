// rv_merge.hip -- merge_consecutive of `reveal transform` (transform.py:713-746): the stage that folds the chain glocalchain leaves into a handful
// of blocks, and the last one that sees the whole list.
//
// The rule (one statement, both programmes below follow it; include/reveal_amd.h has it in full).  The list = the rows sel names, in that order.
// R = the list stably sorted by s1.  qinv[i] = the rank of R[i] in the stable sort of R by s2.  R[i] joins R[i-1] iff their ctgid are equal and
// either both have o = 0 and qinv[i] = qinv[i-1] + 1, or both have o = 1 and qinv[i] = qinv[i-1] - 1 (mrg_joins, rv_merge.h).  A maximal run with
// head h and tail t is the block (s1_h, e1_t, o_h = 0 ? s2_h : s2_t, o_h = 0 ? e2_t : e2_h, o_h, sum of scores, refid_h, ctgid_h); the runs stay in
// the order of R.  A list of fewer than two blocks is returned as it is.
//
// Device programme: k_mrg_gather (only with sel) -> k_mrg_keys (s1, entry number) -> rv_radix_sort_pairs -> k_mrg_keys (s2 of R[i], i) ->
// rv_radix_sort_pairs -> k_mrg_qinv (scatter of the ranks) -> k_mrg_heads (an entry and the one in front of it) -> rv_exclusive_sum_u32 of the
// heads (run numbers) and rv_exclusive_sum_u64 of the scores (a run's score = a difference) -> k_mrg_starts -> k_mrg_emit (one thread per run:
// its head and its tail).  Nothing walks the members of a run and nothing is ordered by an atomic.  The runs are written with the run count as
// the columns' stride, so the merged list comes back in one copy behind the count.
#include "rv_merge.h"
#include <algorithm>
#include <numeric>

namespace {

// eight columns of `stride` rows in one buffer: five int64 arrays, then three int32 arrays
struct MrgCols {
    int64_t *s1, *e1, *s2, *e2, *score; int32_t *o, *refid, *ctgid;
    __host__ __device__ MrgCols(void *p, size_t stride) {
        s1 = (int64_t *)p; e1 = s1 + stride; s2 = e1 + stride; e2 = s2 + stride; score = e2 + stride;
        o = (int32_t *)(score + stride); refid = o + stride; ctgid = refid + stride;
    }
};
constexpr size_t MRG_ROW = 5 * 8 + 3 * 4;      // bytes of a row over the eight columns

__global__ __launch_bounds__(256) void k_mrg_gather(u32 m, const int32_t *__restrict__ sel, const void *src, size_t n, void *dst) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= m) return;
    const MrgCols a(const_cast<void *>(src), n); MrgCols w(dst, m);
    const size_t r = (size_t)sel[i];
    w.s1[i] = a.s1[r]; w.e1[i] = a.e1[r]; w.s2[i] = a.s2[r]; w.e2[i] = a.e2[r]; w.score[i] = a.score[r];
    w.o[i] = a.o[r]; w.refid[i] = a.refid[r]; w.ctgid[i] = a.ctgid[r];
}

// perm == NULL: keys[i] = col[i];  otherwise keys[i] = col[perm[i]] (the column in the order of an earlier sort).  vals[i] = i.
__global__ __launch_bounds__(256) void k_mrg_keys(u32 m, const int64_t *__restrict__ col, const u32 *__restrict__ perm, u64 *__restrict__ keys, u32 *__restrict__ vals) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= m) return;
    keys[i] = (u64)col[perm ? perm[i] : i];
    vals[i] = i;
}

// order2[r] = the position in R of the entry with rank r in the query order
__global__ __launch_bounds__(256) void k_mrg_qinv(u32 m, const u32 *__restrict__ order2, u32 *__restrict__ qinv) {
    const u32 r = blockIdx.x * 256u + threadIdx.x;
    if (r >= m) return;
    qinv[order2[r]] = r;
}

// head[i] = 1 where R[i] starts a run; sc[i] = its score; both arrays get a zero at [m] for the sums
__global__ __launch_bounds__(256) void k_mrg_heads(u32 m, MrgCols c, const u32 *__restrict__ perm, const u32 *__restrict__ qinv, u32 *__restrict__ head, u64 *__restrict__ sc) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= m) return;
    const u32 r = perm[i];
    u32 h = 1;
    if (i > 0) {
        const u32 p = perm[i - 1];
        if (mrg_joins(c.ctgid[p], c.o[p], (int64_t)qinv[i - 1], c.ctgid[r], c.o[r], (int64_t)qinv[i])) h = 0;
    }
    head[i] = h; sc[i] = (u64)c.score[r];
    if (i == 0) { head[m] = 0; sc[m] = 0; }
}

// rnum = exclusive sum of head over m + 1 entries: start[c] = the position in R of the head of run c, start[number of runs] = m
__global__ __launch_bounds__(256) void k_mrg_starts(u32 m, const u32 *__restrict__ rnum, u32 *__restrict__ start, u32 *__restrict__ hdr) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= m) return;
    const u32 c = rnum[i];
    if (rnum[i + 1] != c) start[c] = i;
    if (i == m - 1) { start[rnum[m]] = m; hdr[0] = rnum[m]; }
}

// one thread per run; the columns of the result have the run count as their stride
__global__ __launch_bounds__(256) void k_mrg_emit(u32 m, MrgCols c, const u32 *__restrict__ perm, const u32 *__restrict__ rnum, const u32 *__restrict__ start,
                                                   const u64 *__restrict__ ssum, void *out) {
    const u32 k = blockIdx.x * 256u + threadIdx.x;
    const u32 runs = rnum[m];
    if (k >= runs) return;
    const u32 f = start[k], e = start[k + 1] - 1u;
    const u32 H = perm[f], T = perm[e];
    MrgCols w(out, runs);
    const int32_t o = c.o[H];
    w.s1[k] = c.s1[H]; w.e1[k] = c.e1[T];
    w.s2[k] = o == 0 ? c.s2[H] : c.s2[T];
    w.e2[k] = o == 0 ? c.e2[T] : c.e2[H];
    w.score[k] = (int64_t)(ssum[e + 1] - ssum[f]);
    w.o[k] = o; w.refid[k] = c.refid[H]; w.ctgid[k] = c.ctgid[H];
}

int bits_of(u64 v) { int b = 0; while (v) { b++; v >>= 1; } return b ? b : 1; }

struct Ev2 {
    hipEvent_t a = nullptr, b = nullptr;
    ~Ev2() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
};

}  // namespace

int rv_merge_validate(const RvMrgIn &in, int64_t *max_s1, int64_t *max_s2) {
    if (in.n < 0 || in.m < 0 || (in.n && (!in.s1 || !in.e1 || !in.s2 || !in.e2 || !in.o || !in.score || !in.refid || !in.ctgid))) { rv_set_error("merge: bad arguments"); return -1; }
    if (!in.sel && in.m != in.n) { rv_set_error("merge: bad arguments"); return -1; }
    if (in.n > 0x7ffffff0ll || in.m > 0x7ffffff0ll) { rv_set_error("merge: more than 2^31 - 16 rows"); return -1; }
    const int64_t lim = (int64_t)1 << 61;
    for (int64_t i = 0; i < in.n; i++) {
        if (in.s1[i] < 0 || in.e1[i] < 0 || in.s2[i] < 0 || in.e2[i] < 0 || in.s1[i] >= lim || in.e1[i] >= lim || in.s2[i] >= lim || in.e2[i] >= lim) {
            rv_set_error("merge: coordinates outside 0 .. 2^61 (row %lld)", (long long)i); return -1;
        }
        if (in.o[i] != 0 && in.o[i] != 1) { rv_set_error("merge: o is 0 or 1 (row %lld)", (long long)i); return -1; }
        if (in.score[i] < 0) { rv_set_error("merge: negative score (row %lld)", (long long)i); return -1; }
    }
    const uint64_t tlim = (uint64_t)1 << 62;
    uint64_t total = 0;
    int64_t a = 0, b = 0;
    for (int64_t i = 0; i < in.m; i++) {
        int64_t r = i;
        if (in.sel) {
            r = in.sel[i];
            if (r < 0 || r >= in.n) { rv_set_error("merge: sel names row %lld of %lld", (long long)r, (long long)in.n); return -1; }
        }
        a = std::max(a, in.s1[r]); b = std::max(b, in.s2[r]);
        total += (uint64_t)in.score[r];
        if (total >= tlim) { rv_set_error("merge: the scores' total reaches 2^62"); return -1; }
    }
    if (max_s1) *max_s1 = a;
    if (max_s2) *max_s2 = b;
    return 0;
}

int rv_merge_device(Workspace &ws, const RvMrgIn &in, int64_t max_s1, int64_t max_s2, int64_t *info, RvMrgOut &out) {
    out.clear();
    if (in.m < 2 || in.n < 1) { rv_set_error("merge: the kernels take lists of two blocks and more"); return -1; }
    const u32 m = (u32)in.m;
    const size_t N = (size_t)in.n, M = (size_t)m, M1 = M + 1;
    hipStream_t q = ws.stream;
    DBuf *B = ws.mrg;
    RV_TRY(B[0].reserve(N * MRG_ROW + M * 4));
    if (in.sel) RV_TRY(B[1].reserve(M * MRG_ROW));
    RV_TRY(B[2].reserve(M1 * 8)); RV_TRY(B[3].reserve(M1 * 8));
    for (int k = 4; k < 8; k++) RV_TRY(B[k].reserve(M1 * 4));
    RV_TRY(B[8].reserve(M * MRG_ROW)); RV_TRY(B[9].reserve(64));
    Ev2 ev;
    if (info) { RV_HIP(hipEventCreate(&ev.a)); RV_HIP(hipEventCreate(&ev.b)); }
    const MrgCols up(B[0].p, N);
    int32_t *dsel = (int32_t *)((char *)B[0].p + N * MRG_ROW);
    RV_HIP(hipMemcpyAsync(up.s1, in.s1, N * 8, hipMemcpyHostToDevice, q)); RV_HIP(hipMemcpyAsync(up.e1, in.e1, N * 8, hipMemcpyHostToDevice, q));
    RV_HIP(hipMemcpyAsync(up.s2, in.s2, N * 8, hipMemcpyHostToDevice, q)); RV_HIP(hipMemcpyAsync(up.e2, in.e2, N * 8, hipMemcpyHostToDevice, q));
    RV_HIP(hipMemcpyAsync(up.score, in.score, N * 8, hipMemcpyHostToDevice, q)); RV_HIP(hipMemcpyAsync(up.o, in.o, N * 4, hipMemcpyHostToDevice, q));
    RV_HIP(hipMemcpyAsync(up.refid, in.refid, N * 4, hipMemcpyHostToDevice, q)); RV_HIP(hipMemcpyAsync(up.ctgid, in.ctgid, N * 4, hipMemcpyHostToDevice, q));
    if (in.sel) RV_HIP(hipMemcpyAsync(dsel, in.sel, M * 4, hipMemcpyHostToDevice, q));
    RV_HIP(hipStreamSynchronize(q));      // (the host arrays are the caller's)
    int64_t launches = 0;
    if (ev.a) RV_HIP(hipEventRecord(ev.a, q));
    const unsigned grid = (unsigned)ceil_div((int64_t)m, 256);
    MrgCols c = up;
    if (in.sel) {
        hipLaunchKernelGGL(k_mrg_gather, dim3(grid), dim3(256), 0, q, m, (const int32_t *)dsel, (const void *)B[0].p, N, B[1].p);
        RV_LAUNCH_CHECK(); launches++;
        c = MrgCols(B[1].p, M);
    }
    const int bits1 = bits_of((u64)max_s1), bits2 = bits_of((u64)max_s2);
    u64 *ka = B[2].as<u64>(), *kb = B[3].as<u64>();
    u32 *va = B[4].as<u32>(), *vb = B[5].as<u32>(), *vc = B[6].as<u32>(), *vd = B[7].as<u32>();
    int f = 0;
    hipLaunchKernelGGL(k_mrg_keys, dim3(grid), dim3(256), 0, q, m, (const int64_t *)c.s1, (const u32 *)nullptr, ka, va);
    RV_LAUNCH_CHECK(); launches++;
    RV_TRY(rv_radix_sort_pairs<u32>(ws, ka, va, kb, vb, (int64_t)m, 0, bits1, &f));
    if (f) std::swap(va, vb);
    const u32 *perm = va;                 // R[i] = entry perm[i]; vb is free
    hipLaunchKernelGGL(k_mrg_keys, dim3(grid), dim3(256), 0, q, m, (const int64_t *)c.s2, perm, ka, vc);
    RV_LAUNCH_CHECK(); launches++;
    RV_TRY(rv_radix_sort_pairs<u32>(ws, ka, vc, kb, vd, (int64_t)m, 0, bits2, &f));
    if (f) std::swap(vc, vd);
    u32 *qinv = vb;
    hipLaunchKernelGGL(k_mrg_qinv, dim3(grid), dim3(256), 0, q, m, (const u32 *)vc, qinv);
    RV_LAUNCH_CHECK(); launches++;
    // the keys and the query order are not read again: ka takes the scores and their sums, vc the heads and the run numbers, vd the runs' heads
    u32 *rnum = vc, *start = vd; u64 *ssum = ka;
    u32 *hdr = B[9].as<u32>();
    hipLaunchKernelGGL(k_mrg_heads, dim3(grid), dim3(256), 0, q, m, c, perm, (const u32 *)qinv, rnum, ssum);
    RV_LAUNCH_CHECK(); launches++;
    RV_TRY(rv_exclusive_sum_u32(ws, rnum, rnum, (int64_t)m + 1));
    RV_TRY(rv_exclusive_sum_u64(ws, ssum, ssum, (int64_t)m + 1));
    hipLaunchKernelGGL(k_mrg_starts, dim3(grid), dim3(256), 0, q, m, (const u32 *)rnum, start, hdr);
    RV_LAUNCH_CHECK(); launches++;
    hipLaunchKernelGGL(k_mrg_emit, dim3(grid), dim3(256), 0, q, m, c, perm, (const u32 *)rnum, (const u32 *)start, (const u64 *)ssum, B[8].p);
    RV_LAUNCH_CHECK(); launches++;
    if (ev.b) RV_HIP(hipEventRecord(ev.b, q));
    u32 runs = 0;
    RV_TRY(rv_read_back(ws, &runs, hdr, 4));
    if (runs < 1 || runs > m) { rv_set_error("merge: inconsistent counts from the device"); return -1; }
    const size_t k = runs;
    std::vector<char> land;
    try { land.resize(k * MRG_ROW); out.resize(k); } catch (...) { rv_set_error("merge: out of host memory"); return -1; }
    RV_HIP(hipMemcpyAsync(land.data(), B[8].p, k * MRG_ROW, hipMemcpyDeviceToHost, q));
    RV_HIP(hipStreamSynchronize(q));
    const MrgCols w(land.data(), k);
    memcpy(out.s1.data(), w.s1, k * 8); memcpy(out.e1.data(), w.e1, k * 8); memcpy(out.s2.data(), w.s2, k * 8); memcpy(out.e2.data(), w.e2, k * 8);
    memcpy(out.score.data(), w.score, k * 8); memcpy(out.o.data(), w.o, k * 4); memcpy(out.refid.data(), w.refid, k * 4); memcpy(out.ctgid.data(), w.ctgid, k * 4);
    if (info) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev.a, ev.b) != hipSuccess) ms = 0;
        info[RV_MRG_ROUTE] = 0; info[RV_MRG_ROWS_IN] = in.m; info[RV_MRG_ROWS_OUT] = (int64_t)k;
        info[RV_MRG_BYTES_UP] = (int64_t)(N * MRG_ROW + (in.sel ? M * 4 : 0)); info[RV_MRG_BYTES_DOWN] = (int64_t)(4 + k * MRG_ROW);
        info[RV_MRG_BITS1] = bits1; info[RV_MRG_BITS2] = bits2; info[RV_MRG_LAUNCHES] = launches; info[RV_MRG_KERNEL_NS] = (int64_t)((double)ms * 1e6);
    }
    return 0;
}

// ---- the host programme: the same rule, two std::stable_sort and one walk ----------------------------------------------------------------------------
int rv_merge_rule_host(const RvMrgIn &in, RvMrgOut &out) {
    out.clear();
    const int64_t m = in.m;
    try {
        auto row = [&](int64_t i) -> int64_t { return in.sel ? (int64_t)in.sel[i] : i; };
        auto push = [&](int64_t H, int64_t T, int64_t score) {
            const int32_t o = in.o[H];
            out.s1.push_back(in.s1[H]); out.e1.push_back(in.e1[T]);
            out.s2.push_back(o == 0 ? in.s2[H] : in.s2[T]); out.e2.push_back(o == 0 ? in.e2[T] : in.e2[H]);
            out.o.push_back(o); out.score.push_back(score); out.refid.push_back(in.refid[H]); out.ctgid.push_back(in.ctgid[H]);
        };
        if (m < 2) {
            for (int64_t i = 0; i < m; i++) push(row(i), row(i), in.score[row(i)]);
            return 0;
        }
        std::vector<int32_t> R((size_t)m), ord((size_t)m), qinv((size_t)m);      // R[i] = the row of the i-th entry by s1
        for (int64_t i = 0; i < m; i++) R[(size_t)i] = (int32_t)row(i);
        std::stable_sort(R.begin(), R.end(), [&](int32_t x, int32_t y) { return in.s1[x] < in.s1[y]; });
        std::iota(ord.begin(), ord.end(), 0);
        std::stable_sort(ord.begin(), ord.end(), [&](int32_t x, int32_t y) { return in.s2[R[(size_t)x]] < in.s2[R[(size_t)y]]; });
        for (int64_t r = 0; r < m; r++) qinv[(size_t)ord[(size_t)r]] = (int32_t)r;
        int64_t H = R[0], score = in.score[R[0]];
        for (int64_t i = 1; i < m; i++) {
            const int64_t r = R[(size_t)i], p = R[(size_t)i - 1];
            if (mrg_joins(in.ctgid[p], in.o[p], qinv[(size_t)i - 1], in.ctgid[r], in.o[r], qinv[(size_t)i])) { score += in.score[r]; continue; }
            push(H, p, score);
            H = r; score = in.score[r];
        }
        push(H, R[(size_t)m - 1], score);
    } catch (...) { rv_set_error("merge: out of host memory"); return -1; }
    return 0;
}
