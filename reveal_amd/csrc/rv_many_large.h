// rv_many_large.h -- the index build of rv_many's rounds of pair jobs above RV_LEAF_N ranks (rv_many_large.hip).
#pragma once
#include "rv_common.h"

// defaults of RV_MANY_LARGE_MAX (ranks of the largest job the large rounds take) and RV_MANY_LARGE_MIN (fewer large jobs than this in a
// call stay ordinary): DESIGN.md "Many small alignments" has the measurements
#define RV_MANY_LARGE_MAX_DEFAULT ((int64_t)1 << 17)
#define RV_MANY_LARGE_MIN_DEFAULT 4

// a pair job of a round: where its two sequences begin in the round's shared text, the first rank of its segment
struct ManyDevJob { int64_t abeg, bbeg, off; int32_t la, lb; };

// scratch of the build, kept by rv_many between calls: 37 B per position (+ the radix sort's digit byte and histograms in the workspace)
struct RvManyLargeBufs {
    DBuf txt, job, key[2], val[2], rank, head, flag;
    void release() { flag.release(); txt.release(); job.release(); key[0].release(); key[1].release(); val[0].release(); val[1].release(); rank.release(); head.release(); }
};

// SA (shared-text positions), LCP and BWT byte of every job's segment [off, off + la + lb + 2), as construct() of the job alone gives them.
// djobs: device, ascending off, the segments back to back over [0, n); maxn: ranks of the largest job.  d_cnt: [0] max LCP, [1] error bits
// (device words, cleared by the caller).  The kernel launches made are added to *launches; they do not depend on the number of jobs.
int rv_many_large_build(Workspace &ws, RvManyLargeBufs &B, const ManyDevJob *djobs, int64_t njobs, int64_t n, int64_t maxn, const uint8_t *T,
                        sa_t *SA, lcp_t *LCP, uint8_t *BWT, u32 *d_cnt, int64_t *launches);
