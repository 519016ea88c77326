// rv_many_scan.hip -- the scans of rv_many_scan: getmums (reveal.c:55-116) and getmultimums (reveal.c:436-580, ismultimum :227-259) over the SA / LCP /
// BWT segments of every job of a round at once.
//
// The handle's own scans (rv_scan.hip) find the sample of a position among handle-wide separators, which a round of many jobs does not have: here a
// position's sample is its sequence among the begins of ITS job (rv_many_scan.h).  Everything else a rank needs is inside its job's segment, and the
// segment ends show in the arrays themselves: the LCP of a job's first rank is 0, so
//   - a rank that closes anything (LCP[u] > LCP[u + 1], LCP[u] >= minl >= 1) is never a job's first rank, and the value behind a job's last rank
//     reads as 0, as the reference has it behind the last rank of an index;
//   - a walk to the left stops at the job's first rank at the latest.
// So the kernels are flat over the ranks of the round, a thread per rank, with no per-job state; only the ranks that close an interval look their job
// up (rv_job_of over the segment offsets).
//
// pair predicate (kind 0, and kind 2 for jobs of two sequences): rank u is a MUM when LCP[u - 1] < LCP[u] > LCP[u + 1], the side bits of the BWT bytes
//   of u - 1 and u differ (one suffix in front of the job's first '$', one behind), and the characters in front differ or the one of the smaller
//   position is N, '$' or lower case.  Record: n = 2, members (0, a), (sample of b, b), a < b.
// multi predicate: the thread of rank u emits the LCP intervals that END at u, deepest first -- their values are the successive smaller LCP values
//   met walking left from u while they stay above LCP[u + 1]; an interval qualifies with minn .. k members, all in different samples (k == 2: the side
//   test), some adjacent pair left-maximal.  The walk ends as soon as an interval has more than k members (at most 64 steps).  Concatenated in rank
//   order this is the reference's emission order (closing rank ascending, then value descending): nothing is sorted.
// output: a count pass leaves records << 38 | members per rank, rv_exclusive_sum_u64 turns them into places, the write pass walks again and writes
//   (it counts what the count pass counted: same code, same data).  No capacity is guessed and no counter is shared.  Member totals are 64-bit words
//   throughout; a round is cut at 2^26 ranks (RV_MANY_SCAN_RANKS) so that the record field beside them holds.
#include "rv_many_scan.h"

namespace {

constexpr int TB = 256;
constexpr u64 MMASK = ((u64)1 << RV_MANY_SCAN_MBITS) - 1;

__device__ inline bool is_lower_c(uint8_t c) { return c >= 'a' && c <= 'z'; }
// reveal.c:81-85: ca is the character in front of the smaller position ('$' stands for "position 0" in the BWT byte)
__device__ inline bool left_maximal(uint8_t ca, uint8_t cb) { return (ca != cb) || ca == 'N' || ca == '$' || is_lower_c(ca); }

// the sequence of the job that holds text position p: the last of its k begins at or in front of p; -1: p lies in front of the job
__device__ inline int seq_of(const int64_t *__restrict__ beg, int k, int64_t p) {
    int lo = 0, hi = k;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (beg[mid] <= p) lo = mid + 1; else hi = mid; }
    return lo - 1;
}

// EMIT false: cnt[u] = records << 38 | members of rank u (u == m: 0, the slot that makes the exclusive sum yield the totals); true: cnt holds the sums
template <bool EMIT>
__global__ __launch_bounds__(TB) void k_many_scan(RvManyScanRound R, u64 *__restrict__ cnt, RvManyScanRec *__restrict__ rec, uint16_t *__restrict__ so,
                                                  u32 *__restrict__ pos, u64 nrec, u64 nmem) {
    const int64_t u = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (u > R.m) return;
    u64 rq = 0, mq = 0;
    const u32 lmin = (u32)(R.minl > 1 ? R.minl : 1);
    const u32 top = u < R.m ? (u32)R.LCP[u] : 0u;
    const u32 lnext = u + 1 < R.m ? (u32)R.LCP[u + 1] : 0u;
    if (top >= lmin && top > lnext) {
        const int j = rv_job_of(R.off, R.njobs, u);
        const int64_t j0 = R.off[j], j1 = R.off[j + 1];
        const int s0 = R.sfirst[j];
        const int k = R.sfirst[j + 1] - s0;
        if (!(j0 >= 0 && j0 < u && u < j1 && j1 <= R.m && s0 >= 0 && k >= 2 && k <= 64 && s0 + k <= R.nbeg)) { atomicOr(R.err, 1u); goto done; }
        const int64_t *beg = R.beg + s0;
        const int32_t *loc = R.loc + s0;
        const u64 rbase = EMIT ? cnt[u] >> RV_MANY_SCAN_MBITS : 0, mbase = EMIT ? cnt[u] & MMASK : 0;
        if (R.kind == 0 || (R.kind == 2 && k == 2)) {
            const uint8_t b0 = R.BWT[u - 1], b1 = R.BWT[u];
            if ((u32)R.LCP[u - 1] < top && ((b0 ^ b1) & RV_BWT_SIDE)) {
                const int64_t p0 = (int64_t)R.SA[u - 1], p1 = (int64_t)R.SA[u];
                const int q0 = seq_of(beg, k, p0), q1 = seq_of(beg, k, p1);
                if (q0 < 0 || q1 < 0) { atomicOr(R.err, 2u); goto done; }
                const int64_t l0 = p0 - beg[q0] + loc[q0], l1 = p1 - beg[q1] + loc[q1];
                const bool first = l0 < l1;      // (rank u - 1 holds the smaller position)
                if (first ? left_maximal(b0 & RV_BWT_CHAR, b1 & RV_BWT_CHAR) : left_maximal(b1 & RV_BWT_CHAR, b0 & RV_BWT_CHAR)) {
                    if (EMIT) {
                        if (rbase >= nrec || mbase + 2 > nmem) { atomicOr(R.err, 4u); goto done; }
                        RvManyScanRec r; r.l = top; r.n = 2; r.moff = mbase;
                        rec[rbase] = r;
                        so[mbase] = (uint16_t)(first ? q0 : q1); pos[mbase] = (u32)(first ? l0 : l1);
                        so[mbase + 1] = (uint16_t)(first ? q1 : q0); pos[mbase + 1] = (u32)(first ? l1 : l0);
                    }
                    rq = 1; mq = 2;
                }
            }
        } else {
            u32 cur = top;
            int64_t p = u;
            while (cur > lnext && cur >= lmin && p > j0) {      // (p == j0 with a value left: the segment does not begin with 0)
                // the interval of value cur that ends at u begins at the first rank to the left whose LCP is below cur
                int64_t lb = p - 1;
                while (lb > j0 && (u32)R.LCP[lb] >= cur) { lb--; if (u - lb + 1 > k) break; }
                const int64_t n = u - lb + 1;
                if (n > k || (u32)R.LCP[lb] >= cur) break;      // every further interval is larger still (or the segment does not begin with 0)
                bool take = n >= (R.minn_k ? (int64_t)k : (int64_t)R.minn);
                if (take) {
                    if (k == 2) take = ((R.BWT[lb] ^ R.BWT[u]) & RV_BWT_SIDE) != 0;
                    else {
                        u64 seen = 0;
                        for (int64_t x = lb; x <= u && take; x++) {
                            const int q = seq_of(beg, k, (int64_t)R.SA[x]);
                            if (q < 0) { atomicOr(R.err, 2u); goto done; }
                            const u64 bit = (u64)1 << q;
                            take = !(seen & bit);
                            seen |= bit;
                        }
                    }
                }
                if (take) {
                    bool lm = false;
                    uint8_t ca = R.BWT[lb] & RV_BWT_CHAR;
                    for (int64_t x = lb; x < u && !lm; x++) {      // reveal.c:246-256
                        const uint8_t cb = R.BWT[x + 1] & RV_BWT_CHAR;
                        lm = cb == '$' || left_maximal(ca, cb);
                        ca = cb;
                    }
                    take = lm;
                }
                if (take) {
                    if (EMIT) {
                        if (rbase + rq >= nrec || mbase + mq + (u64)n > nmem) { atomicOr(R.err, 4u); goto done; }
                        RvManyScanRec r; r.l = cur; r.n = (u32)n; r.moff = mbase + mq;
                        rec[rbase + rq] = r;
                        for (int64_t x = lb; x <= u; x++) {
                            const int64_t px = (int64_t)R.SA[x];
                            const int q = seq_of(beg, k, px);
                            if (q < 0) { atomicOr(R.err, 2u); goto done; }
                            so[mbase + mq + (u64)(x - lb)] = (uint16_t)q;
                            pos[mbase + mq + (u64)(x - lb)] = (u32)(px - beg[q] + loc[q]);
                        }
                    }
                    rq++; mq += (u64)n;
                }
                cur = (u32)R.LCP[lb];      // the value of the enclosing interval
                p = lb;
            }
        }
    }
done:
    if (!EMIT) cnt[u] = rq << RV_MANY_SCAN_MBITS | mq;
}

// first[j] = the sums at job j's first rank, first[njobs] = the totals
__global__ __launch_bounds__(TB) void k_many_scan_first(const u64 *__restrict__ cnt, const int64_t *__restrict__ off, int njobs, int64_t m, u64 *__restrict__ first,
                                                        u32 *__restrict__ err) {
    const int j = (int)(blockIdx.x * TB + threadIdx.x);
    if (j > njobs) return;
    const int64_t o = off[j];
    const bool ok = o >= 0 && o <= m && (j < njobs || o == m) && (j == 0 ? o == 0 : off[j - 1] < o);
    if (!ok) atomicOr(err, 1u);
    first[j] = ok ? cnt[o] : 0;
}

}  // namespace

int rv_many_scan_count(Workspace &ws, const RvManyScanRound &R, u64 *cnt, u64 *first, int64_t *launches) {
    if (R.m < 1 || R.m > RV_MANY_SCAN_RANKS || R.njobs < 1) { rv_set_error("rv_many_scan: a round of %lld ranks and %d jobs", (long long)R.m, R.njobs); return -1; }
    hipLaunchKernelGGL((k_many_scan<false>), dim3((unsigned)ceil_div(R.m + 1, TB)), dim3(TB), 0, ws.stream, R, cnt, (RvManyScanRec *)nullptr, (uint16_t *)nullptr,
                       (u32 *)nullptr, (u64)0, (u64)0);
    RV_LAUNCH_CHECK();
    RV_TRY(rv_exclusive_sum_u64(ws, cnt, cnt, R.m + 1));
    hipLaunchKernelGGL(k_many_scan_first, dim3((unsigned)ceil_div((int64_t)R.njobs + 1, TB)), dim3(TB), 0, ws.stream, cnt, R.off, R.njobs, R.m, first, R.err);
    RV_LAUNCH_CHECK();
    // (rv_prims.hip scan_rec: one launch up to a tile of 2048 words, two more per further level)
    if (launches) *launches += 2 + (R.m + 1 <= 2048 ? 1 : R.m + 1 <= (int64_t)2048 * 2048 ? 3 : 5);
    return 0;
}

int rv_many_scan_write(Workspace &ws, const RvManyScanRound &R, const u64 *cnt, RvManyScanRec *rec, u64 nrec, uint16_t *so, u32 *pos, u64 nmem, int64_t *launches) {
    if (!nrec) return 0;
    hipLaunchKernelGGL((k_many_scan<true>), dim3((unsigned)ceil_div(R.m + 1, TB)), dim3(TB), 0, ws.stream, R, (u64 *)cnt, rec, so, pos, nrec, nmem);
    RV_LAUNCH_CHECK();
    if (launches) *launches += 1;
    return 0;
}
