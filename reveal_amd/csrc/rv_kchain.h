// rv_kchain.h -- the collinear chain of `reveal chain` (reveal/chain.py:214-314) over the full multi-MUMs of every job of one of rv_many's scan rounds
// (rv_kchain.hip): k_many_kchain on the records the write pass of rv_many_scan.hip has left in device memory, and rv_kchain, the host restatement.
#pragma once
#include "rv_common.h"
#include "rv_many_scan.h"

#define RV_KCHAIN_MEMBERS 2048      // members (records x k) of the largest job the kernel takes: its points in LDS, 32 bits each
#define RV_KCHAIN_CAP 1024          // ... and its records
#define RV_KCHAIN_WMAX ((int64_t)1 << 20)      // weights up to this: 2^20 x 2^17 positions x 2016 pairs x 1024 nodes stays below 2^63
#define RV_KCHAIN_FLAG 4u           // rv_many_flagged bit of a job the kernel gives back to rv_kchain on the host

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

// the chains of every job of the round: one workgroup per job.  Launches: 1, added to *launches
int rv_many_kchain_run(Workspace &ws, const RvManyScanRound &R, const RvKchainRound &K, const RvKchainArgs &A, int64_t *launches);
// after the exclusive sum over K.nodes: cfirst[j] = the sums at job j's first rank, cfirst[njobs] = the totals.  Launches: 1
int rv_many_kchain_first(Workspace &ws, const RvManyScanRound &R, const RvKchainRound &K, u64 *cfirst, int64_t *launches);
// the paths into CSR arrays: l / score per node, pos k per node (relative to each sequence's begin).  Launches: 1
int rv_many_kchain_write(Workspace &ws, const RvManyScanRound &R, const RvKchainRound &K, const u64 *cfirst, u32 *out_l, int64_t *out_score, u32 *out_pos,
                         u64 nnodes, u64 nmem, int64_t *launches);
