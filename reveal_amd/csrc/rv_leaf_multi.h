// rv_leaf_multi.h -- host interface of the leaf kernel for jobs of several samples (rv_leaf_multi.hip)
#pragma once
#include "rv_common.h"
#include "rv_leaf.h"

#define RV_MANY_KMAX 16        // samples of a job the kernel's narrow form takes (one interval per sample and frame)
#define RV_MANY_WIDE_KMAX 64   // ... its wide form (RV_MANY_WIDE): lane s of a wavefront owns sample s, the sample id has six bits of the
                               // `smp` byte, and the level pipeline's multi-sample scan keeps a one-word census up to 64 samples (rv_scan.hip)

// a job of rv_many: k sequences, every one a sample, `s0$s1$..s(k-1)$` contiguous in the round's text; its n <= RV_LEAF_N ranks
// lie at the same offset of the index arrays
struct RvLeafMultiJob { int64_t beg; int32_t n, pad; };

// anchor k of a launch: length l, n members an_pos[moff .. moff + n) ascending, positions local to job `job`
struct RvLeafMultiAnchor { u32 l, job, n, moff; };

struct RvLeafMultiArgs {
    const RvLeafMultiJob *jobs;
    const sa_t *SA; const lcp_t *LCP; const uint8_t *BWT;    // of the round (read only); SA in positions of the round's text
    uint8_t *T;                                              // the round's text: the kernel lower-cases what it anchors
    int minl, minn;
    u32 stage_cap;                                           // anchors a workgroup stages in LDS before it writes them out (<= 256)
    unsigned long long *count;                               // anchors << 32 | members: one reservation takes both
    u32 anchor_cap, member_cap;
    RvLeafMultiAnchor *anchors; uint16_t *an_pos;
    unsigned long long *stats;                               // [0] sub-indices visited, [1] anchors, [2] anchored bp, [3] max depth
    u32 *err;                                                // 4: stack full, 8: a sub-index is not the suffixes of its intervals, 16: a bad job, 32: output full
};

// kmax: RV_MANY_KMAX or RV_MANY_WIDE_KMAX -- the form of the kernel; every job of the launch has at most that many samples
int rv_leaf_multi_launch(hipStream_t q, const RvLeafMultiArgs &a, int njobs, int kmax);

// k_leaf_multi_chain (rv_leaf_multi_chain.hip): the same jobs -- 3 .. RV_MANY_KMAX samples in the narrow form, up to RV_MANY_WIDE_KMAX in the wide one, at
// most RV_LEAF_N ranks -- with the reference's default picker (schemes.graphmumpicker; rv_pick_chain for any number of samples) as the pick stage, for
// rv_many's RV_MANY_CHAIN_MULTI and RV_MANY_CHAIN_WIDE rounds.  What the caller must have checked (rv_many.hip many_class_admits, the
// two rows of many_classes): trim on, minl > 0, no seeds, a --maxmums that cannot bite, weights within RV_LEAF_MCHAIN_WMAX.
#define RV_LEAF_MCHAIN_WMAX 1024       // rv_leaf_multi_chain.hip derives it for both forms: scores of up to 16 / 64 paths in 32 bits
struct RvLeafMultiChainArgs {
    int32_t wscore, wpen;                                    // 0 .. RV_LEAF_MCHAIN_WMAX
    int gcmodel;                                             // 0 sumofpairs, 1 star-avg, 2 star-med
    u32 *flags;                                              // one word per job, zeroed by the caller: != 0 -- the job was not finished here (1: the reference's own
                                                             // trim_overlap raises, 2: broken chain, 8: two matches share the split's offsets, 16: rv_many's test hook, 32: frame stack full)
};
// kmax: RV_MANY_KMAX or RV_MANY_WIDE_KMAX -- the form of the kernel, as for rv_leaf_multi_launch
int rv_leaf_multi_chain_launch(hipStream_t q, const RvLeafMultiArgs &a, const RvLeafMultiChainArgs &c, int njobs, int kmax);
