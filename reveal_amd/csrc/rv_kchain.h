// rv_kchain.h -- the collinear chain of `reveal chain` (reveal/chain.py:214-314) over the full multi-MUMs of every job of one of rv_many's scan rounds
// (rv_kchain.hip): k_many_kchain on the records the write pass of rv_many_scan.hip has left in device memory, and rv_kchain, the host restatement.
#pragma once
#include "rv_common.h"
#include "rv_many_scan.h"

#define RV_KCHAIN_MEMBERS 2048      // members (records x k) of the largest job the kernel takes: its points in LDS, 32 bits each
#define RV_KCHAIN_CAP 1024          // ... and its records
#define RV_KCHAIN_WMAX ((int64_t)1 << 20)      // weights up to this: 2^20 x 2^17 positions x 2016 pairs x 1024 nodes stays below 2^63
#define RV_KCHAIN_FLAG 4u           // rv_many_flagged bit of a job the kernel gives back to rv_kchain on the host
// The programme in device memory (rv_kchain_big.hip) holds 64-bit scores too, and 32-bit positions relative to each sequence's begin.  Every score is the
// score of a path whose nodes lie inside their sequences and, by admissibility, do not overlap in any of them.  Along such a path the lengths sum to at
// most min len, so the gains sum to at most wscore x k(k-1)/2 x min len.  A step's gap cost is at most (k-1) x sum_d D_d <= k(k-1)/2 x sum_d D_d under
// every model (sumofpairs: |D_i - D_j| <= D_i + D_j over the pairs; star-avg and star-med: at most max D), and the D_d of the steps of a path sum to at
// most len_d + 1 (from p1 = -1 to p2 = len_d), so the gap costs sum to at most wpen x k(k-1)/2 x sum_d (len_d + 1).  An offer is such a score plus one
// more gain and minus one more cost of the same path.  A list is admitted when 2 x (gains + costs) < 2^62: no sum or difference of two scores leaves 64 bits.
#ifndef RV_KCHAIN_BIG_TILE
#define RV_KCHAIN_BIG_TILE 64               // targets of a tile = threads of a workgroup of the step kernel (64, 128 or 256; 256 was tried: profiles/kchain_big.txt)
#endif
#define RV_KCHAIN_BIG_CAP ((int64_t)1 << 20)      // kept points of the longest list the device programme takes
#define RV_KCHAIN_BIG_MEMBERS ((int64_t)1 << 24)  // ... and its members (points x k)
#define RV_KCHAIN_BIG_MIN_DEFAULT 512       // kept points from which a list no round has chained goes to the device programme: the smallest measured size
                                            // from which it beats the host programme for k = 2 by more than both spreads (profiles/kchain_big.txt)
#define RV_KCHAIN_BIG_SCORE ((int64_t)1 << 62)
// why the preparation leaves a list to the host programme (rv_kchain_admit; 0: the device programme takes it)
#define RV_KCHAIN_REFUSE_L0 1          // a record of length 0
#define RV_KCHAIN_REFUSE_SHARED 2      // a coordinate shared by two points in some dimension
#define RV_KCHAIN_REFUSE_BITS 4        // a length or a position that needs more than 31 bits, or a point outside its sequence
#define RV_KCHAIN_REFUSE_CAP 8         // more than RV_KCHAIN_BIG_CAP points or RV_KCHAIN_BIG_MEMBERS members
#define RV_KCHAIN_REFUSE_K 16          // more than 64 sequences
#define RV_KCHAIN_REFUSE_SCORE 32      // scores that might leave 64 bits

struct RvKchainArgs { int64_t maxmums, wpen, wscore; int gcmodel; int cap; };

// Device buffers of a round's chains.  stage_*: a slot per record of the round (a job's path fits the room of its records); nodes: m + 1 words, zero
// but for nodes << RV_MANY_SCAN_MBITS | nodes * k at each job's first rank, so that the sum over the ranks -- never over the jobs -- places the paths;
// flag / end: a word per job; err: bit 1 a descriptor outside the round, 2 a member outside its job, 4 a path outside its room
struct RvKchainRound {
    const RvManyScanRec *rec; const uint16_t *so; const u32 *pos; u64 nrec, nmem;
    const u64 *first;             // the scan's sums at the jobs' first ranks (rv_many_scan_count)
    u32 *stage_rec; int64_t *stage_score;
    u64 *nodes; u32 *flag; int64_t *end; u32 *err;
};

// utils.gapcost (utils.py:162-183) for both kernels: a(i), b(i) give coordinate i of the two points (KcP1: p1 = (-1, ..)).  Python 2's floor division
// for star-avg (the operand is not negative), selection by counting for star-med
struct KcStrided { const u32 *p; int64_t stride; __device__ int64_t operator()(int i) const { return (int64_t)p[(int64_t)i * stride]; } };
struct KcP1 { __device__ int64_t operator()(int) const { return -1; } };
template <class PA, class PB> __device__ inline int64_t kc_gap(const PA &a, const PB &b, int k, int model) {
#define KC_D(i) (a(i) - b(i))
    if (model == 1) {
        int64_t s = 0;
        for (int i = 0; i < k; i++) s += KC_D(i);
        return (s < 0 ? -s : s) / k;
    }
    if (model == 2) {      // sorted(D)[k / 2]: the value with k / 2 values in front of it, equal ones counted by index
        for (int i = 0; i < k; i++) {
            int64_t di = KC_D(i); di = di < 0 ? -di : di;
            int before = 0;
            for (int j = 0; j < k; j++) { int64_t dj = KC_D(j); dj = dj < 0 ? -dj : dj; before += (dj < di || (dj == di && j < i)) ? 1 : 0; }
            if (before == k / 2) return di;
        }
        return 0;
    }
    int64_t p = 0;
    for (int i = 0; i < k; i++) {
        int64_t di = KC_D(i); di = di < 0 ? -di : di;
        for (int j = i + 1; j < k; j++) { int64_t dj = KC_D(j); dj = dj < 0 ? -dj : dj; const int64_t d = di - dj; p += d < 0 ? -d : d; }
    }
    return p;
#undef KC_D
}

// the chains of every job of the round: one workgroup per job.  Launches: 1, added to *launches
int rv_many_kchain_run(Workspace &ws, const RvManyScanRound &R, const RvKchainRound &K, const RvKchainArgs &A, int64_t *launches);
// after the exclusive sum over K.nodes: cfirst[j] = the sums at job j's first rank, cfirst[njobs] = the totals.  Launches: 1
int rv_many_kchain_first(Workspace &ws, const RvManyScanRound &R, const RvKchainRound &K, u64 *cfirst, int64_t *launches);
// the paths into CSR arrays: l / score per node, pos k per node (relative to each sequence's begin).  Launches: 1
int rv_many_kchain_write(Workspace &ws, const RvManyScanRound &R, const RvKchainRound &K, const u64 *cfirst, u32 *out_l, int64_t *out_score, u32 *out_pos,
                         u64 nnodes, u64 nmem, int64_t *launches);
