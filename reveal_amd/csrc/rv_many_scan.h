// rv_many_scan.h -- MUM / multi-MUM lists of every job of one of rv_many's rounds (rv_many_scan.hip).
#pragma once
#include "rv_common.h"

// A round as its index build leaves it: SA, LCP and BWT segments back to back over [0, m), segment j = [off[j], off[j + 1]), off[njobs] = m,
// LCP[off[j]] == 0.  Job j has k = sfirst[j + 1] - sfirst[j] sequences (2 .. 64); sequence q of it begins at text position beg[sfirst[j] + q]
// (increasing with q) and at position loc[sfirst[j] + q] of the job's stand-alone text s0$s1$..: a text position p of the job lies in the last
// sequence that begins at or in front of it, at the stand-alone coordinate p - beg + loc.  Every layout the rounds have fits: job-contiguous
// (beg - loc the same for all q), the pair layout and the sample-major one.  All pointers are device memory.
struct RvManyScanRound {
    const sa_t *SA; const lcp_t *LCP; const uint8_t *BWT; int64_t m;
    const int64_t *off; const int32_t *sfirst; const int64_t *beg; const int32_t *loc;
    int njobs, nbeg;
    int minl, minn, kind;      // kind 0: getmums, 1: getmultimums, 2: getmums for the jobs of two sequences, getmultimums for the rest
    int minn_k;                // 1: every job's minn is its number of sequences (rv_many_kchain), whatever minn says
    u32 *err;                  // error bits: 1 a job descriptor outside the round, 2 a position outside its job's sequences, 4 a record outside the counted room
};
// a record of the lists: value, members, first member in so[] / pos[] (counted over the round)
struct RvManyScanRec { u32 l, n; u64 moff; };
// counts of a rank, and their running sums: records << RV_MANY_SCAN_MBITS | members.  A record has at most 64 members and a round fewer records than
// ranks, so with at most RV_MANY_SCAN_RANKS ranks a round the members stay below 2^32 and the records below 2^26: both fields hold
#define RV_MANY_SCAN_MBITS 38
#define RV_MANY_SCAN_RANKS ((int64_t)1 << 26)

// count pass over the m ranks, exclusive sum, and the sums at the jobs' first ranks: first[j] = what the jobs in front of j hold, first[njobs] = the
// round's totals.  cnt: m + 1 words (device), first: njobs + 1 words (device).  The launches made (3, 5 or 7 by m, never by the number of jobs) are
// added to *launches
int rv_many_scan_count(Workspace &ws, const RvManyScanRound &R, u64 *cnt, u64 *first, int64_t *launches);
// write pass: the same walk again, every rank's records at the place the sums give it -- rank order, and inside a rank the deepest interval first:
// the reference's emission order.  pos[]: stand-alone coordinates of the job
int rv_many_scan_write(Workspace &ws, const RvManyScanRound &R, const u64 *cnt, RvManyScanRec *rec, u64 nrec, uint16_t *so, u32 *pos, u64 nmem, int64_t *launches);
