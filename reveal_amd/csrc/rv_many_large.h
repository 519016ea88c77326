// rv_many_large.h -- the index build of rv_many's rounds of pair jobs above RV_LEAF_N ranks (rv_many_large.hip).
#pragma once
#include "rv_common.h"
#include "rv_leaf_multi.h"      // RV_MANY_KMAX, RV_MANY_WIDE_KMAX

// defaults of RV_MANY_LARGE_MAX (ranks of the largest job the large rounds take) and RV_MANY_LARGE_MIN (fewer large jobs than this in a
// call stay ordinary): DESIGN.md "Many small alignments" has the measurements
#define RV_MANY_LARGE_MAX_DEFAULT ((int64_t)1 << 17)
#define RV_MANY_LARGE_MIN_DEFAULT 4
// default of RV_MANY_CHAIN_LARGE_MULTI_MIN (fewer admitted jobs of 3 .. 16 sequences above RV_LEAF_N ranks in a call under a picker stay ordinary): the smallest
// count measured at which the shared rounds win (profiles/many_chain_large_multi.txt: one job loses, 5.6 against 3.6 ms; four win, 11.2 against 17.4 ms).  Not
// RV_MANY_LARGE_MULTI_MIN's 16: the ordinary path costs 4 - 5 ms a job under a picker, 0.8 ms without
#define RV_MANY_CHAIN_LARGE_MULTI_MIN_DEFAULT 4
// default of RV_MANY_CHAIN_WIDE_LARGE_MIN (fewer admitted jobs of 17 .. 64 sequences above RV_LEAF_N ranks in a call under a picker stay ordinary): the smallest
// count measured at which the shared rounds win (profiles/many_chain_wide_large.txt, jobs of 32 sequences: one job ties, 3.0 against 3.0 ms; two win, 3.4
// against 5.8 ms, far outside both spreads of 0.1 ms).  Lower than RV_MANY_CHAIN_LARGE_MULTI_MIN's 4: a round of a job or two costs 3 ms here, 5 - 8 ms there
#define RV_MANY_CHAIN_WIDE_LARGE_MIN_DEFAULT 2
#define RV_MANY_CHAIN_LARGE_MIN_DEFAULT 4      // RV_MANY_CHAIN_LARGE_MIN: fewer admitted pair jobs above RV_LEAF_N ranks in a call under a picker stay ordinary
// default of RV_MANY_WIDE_LARGE_MIN (fewer jobs of 17 .. 64 sequences above RV_LEAF_N ranks than this in a call stay ordinary): the smallest
// count measured at which the shared rounds are not slower at k = 17, 32 and 64 (profiles/many_wide.txt: 4 jobs of 32 sequences tie, 8 win)
#define RV_MANY_WIDE_LARGE_MIN_DEFAULT 8
// default of RV_MANY_SCAN_LARGE_MIN (fewer admitted jobs above RV_LEAF_N ranks than this in a call of rv_many_scan stay ordinary): the smallest count measured at
// which the shared rounds are not slower for pair jobs and for jobs of 8 sequences (profiles/many_mums_large.txt: a round costs 1.1 - 1.3 ms whatever it holds; one job
// loses, 1.09 against 0.38 ms and 1.24 against 0.65 ms; two lose or tie, 1.14 against 0.75 and 1.29 against 1.25 ms; four win, 1.38 against 1.48 and 1.57 against 2.51 ms)
#define RV_MANY_SCAN_LARGE_MIN_DEFAULT 4

// a pair job of a round: where its two sequences begin in the round's shared text, the first rank of its segment
struct ManyDevJob { int64_t abeg, bbeg, off; int32_t la, lb; };

// a job of k = 3 .. RV_MANY_WIDE_KMAX sequences of a sample-major round (RV_MANY_LARGE_MULTI: up to RV_MANY_KMAX; RV_MANY_WIDE: above): sample q of the round's text holds the q-th sequence of
// every job that has one.  off: the first rank of its segment; n: its ranks (sum of lengths + k); beg[q]: where sequence q begins in the shared
// text; pend[q]: the end of sequence q's local prefix, lengths + 1 accumulated -- sequence q and its '$' are the local positions
// [pend[q - 1], pend[q]) of the stand-alone text s0$s1$..s(k-1)$, and pend[k - 1] = n
struct ManyDevJobK { int64_t off; int64_t beg[RV_MANY_WIDE_KMAX]; int32_t pend[RV_MANY_WIDE_KMAX]; int32_t k, n; };

// a job of k = 2 .. RV_MANY_WIDE_KMAX sequences of a job-contiguous round (the scan rounds of rv_many_scan above RV_LEAF_N ranks): the job lies in the
// round's text as its stand-alone text s0$s1$..s(k-1)$ at [off, off + n), which is its segment of ranks as well.  la: the length of its first sequence
// (the side bit of a BWT byte says "behind the job's first '$'", for every k).  The build needs nothing else: 16 bytes a job, against 784 of ManyDevJobK
struct ManyDevJobC { int64_t off; int32_t n, la; };

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
// the same for jobs of 3 .. RV_MANY_WIDE_KMAX sequences in the sample-major layout: segment [off, off + n) of a job = construct() of its stand-alone text
// s0$s1$..s(k-1)$, SA in shared-text positions.  nT: bytes of T (a descriptor that points outside it is refused through d_cnt[1], not read).
int rv_many_large_build_k(Workspace &ws, RvManyLargeBufs &B, const ManyDevJobK *djobs, int64_t njobs, int64_t n, int64_t maxn, const uint8_t *T, int64_t nT,
                          sa_t *SA, lcp_t *LCP, uint8_t *BWT, u32 *d_cnt, int64_t *launches);
// the same for jobs of 2 .. RV_MANY_WIDE_KMAX sequences in the job-contiguous layout: T holds the n bytes of the round, job j's stand-alone text at
// [off, off + n_j), and the build works on T in place (nothing is gathered: B.txt stays unused).  The keys and the LCP loop read eight bytes at a time,
// so the caller keeps 64 zero bytes behind T[n - 1].  SA in positions of T (job-local: SA - off).  A descriptor that is not back to back with its
// neighbours, has n < 4 or la outside 1 .. n - 3, or whose text has no '$' at la and at n - 1 is refused through d_cnt[1]; nothing outside T is read.
int rv_many_large_build_c(Workspace &ws, RvManyLargeBufs &B, const ManyDevJobC *djobs, int64_t njobs, int64_t n, int64_t maxn, const uint8_t *T,
                          sa_t *SA, lcp_t *LCP, uint8_t *BWT, u32 *d_cnt, int64_t *launches);
