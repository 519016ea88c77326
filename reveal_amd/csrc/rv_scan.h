// rv_scan.h -- scan kernels' host interface (see rv_scan.hip)
#pragma once
#include "rv_common.h"

#ifndef RV_PAIR_TILE
#define RV_PAIR_TILE 1024    // ranks per tile of the pair scan = what one wave scans (sixteen per lane)
#endif
#define RV_TSUB_TILE 2048    // granularity of the tile -> sub-index tables the host ships (== RV_SPLIT_TILE)

// one pairwise MUM: a < b text positions, l = LCP[rank], rank inside the
// scanned (concatenated) array
struct RvPairRec {
    sa_t a, b;
    u32  l;
    u32  rank;
};

#define RV_PAIR_SLOTS 16
// Streams SA/LCP/BWT[0..m) once.  The first RV_PAIR_SLOTS survivors of tile t
// (1024 ranks, rank order) go to slots[t*RV_PAIR_SLOTS ..], further ones to
// ovf[tileovf[t] ..] (*ovf_counter must be zero: rv_pair_compact_launch leaves it so);
// tilecnt[t] = number of survivors, tilecnt[ntile] = 0.  rv_pair_compact_launch packs them densely in rank order given
// tileoff = exclusive scan of tilecnt.
// nsubs > 0: also initialises the tables of the device-side picker (best, picks) that rv_pick_slots_launch fills.
// wit given (the anchor cascade's top-level scan): the scan also lists the repeat witnesses of k_cas_witness (rv_cascade.hip), in any order, in
// RV_WIT_REGIONS regions of cap entries each: entry i of region r at r * cap + i, counters[r] (zeroed by the caller) counts also what did not fit.
// A workgroup's RV_PAIR_WG_TILE ranks go to one region, region = workgroup mod RV_WIT_REGIONS.
#define RV_WIT_REGIONS 64
#define RV_PAIR_WG_TILE (4 * RV_PAIR_TILE)
struct RvScanWit { sa_t *pos; u32 *val; u32 *rank; u32 cap; u32 *counters; };
int rv_scan_pair_launch(Workspace &ws, const sa_t *SA, const lcp_t *LCP, int64_t m, const uint8_t *BWT, sa_t nsep0, int minl,
                        RvPairRec *slots, RvPairRec *ovf, u32 ovf_cap, u32 *ovf_counter, u32 *tilecnt, u32 *tileovf,
                        unsigned long long *best, RvPairRec *picks, int nsubs,
                        hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr,    // both given: the kernel's own start / stop (hipExtLaunchKernelGGL)
                        const RvScanWit *wit = nullptr);
// built-in picker straight from the slots (no compaction): picks[0] = header {0, overflow count, *err, 0}, picks[1+s] = longest
// record of sub-index s (smallest a on ties), rank 0xFFFFFFFF = none; resets *ovf_counter
int rv_pick_slots_launch(Workspace &ws, const RvPairRec *slots, const RvPairRec *ovf, u32 ovf_cap, const u32 *tilecnt, const u32 *tileovf, int64_t ntile,
                         const int64_t *sub_start, int nsubs, unsigned long long *best, RvPairRec *picks, u32 *ovf_counter, const u32 *err,
                         const int *tile_sub, int64_t ntsub);      // tile_sub (optional): sub-index of the first rank of every RV_TSUB_TILE ranks
// The reference's default picker in place of the longest record (k_pick_chain, rv_pick_chain.hip; rv_many's handle under the chain route): picks[1 + s] =
// the TRIMMED match schemes.graphmumpicker splits sub-index s on (its rank field: the sub-index' first rank), for every sub-index whose flag byte has
// bit 0 clear; same header, same reset of *ovf_counter.  nodes: a0, a1, b0, b1 per sub-index and flags: one byte per sub-index, as k_decide reads them.
// A sub-index the kernel cannot decide sets bits in the flag word of its JOB (job_begin: the ascending begins of the jobs' first sequences in the text,
// njobs of them) and gets no pick: 1 the reference's own trim_overlap raises, 2 broken chain or a match outside the intervals, 32 more than `cap`
// candidates, 64 an interval of 2^17 positions or more.  cap: at most RV_PICK_CHAIN_CAP_MAX (RV_PICK_CHAIN_CAP lowers it: test hook).
#define RV_PICK_CHAIN_CAP_MAX 1024
#define RV_PICK_CHAIN_WMAX 1024
#define RV_PICK_CHAIN_RANKS (1 << 17)
struct RvPickChainArgs {
    const sa_t *nodes; const uint8_t *flags;
    int32_t wscore, wpen;                                    // 0 .. RV_PICK_CHAIN_WMAX
    int gcmodel;                                             // 0 sumofpairs, 1 star-avg, 2 star-med
    u32 cap;
    u32 *job_flags; const int64_t *job_begin; int njobs;
};
int rv_pick_chain_launch(Workspace &ws, const RvPairRec *slots, const RvPairRec *ovf, u32 ovf_cap, const u32 *tilecnt, const u32 *tileovf, int64_t ntile,
                         const int64_t *sub_start, int nsubs, RvPairRec *picks, u32 *ovf_counter, const u32 *err, const RvPickChainArgs &c);
// out holds RV_PAIR_HDR header records ({total, overflow count, *err, 0} as u32) followed by the packed records.
// Resets *ovf_counter for the next scan.
#define RV_PAIR_HDR 1
int rv_pair_compact_launch(Workspace &ws, const RvPairRec *slots, const RvPairRec *ovf, const u32 *tilecnt, const u32 *tileovf,
                           const u32 *tileoff, int64_t ntile, RvPairRec *out, u32 out_cap, u32 *ovf_counter, const u32 *err, u32 ovf_cap);

#define RV_MULTI_TILE 512    // ranks per tile of the multi-MUM scan = what one wave scans
struct RvMultiRec { u32 l, n, ub, pad; };
// Multi-MUM scan (getmultimums, reveal.c:436-580).  Records and members of
// tile t (512 ranks) land at rec[tab.x .. +tab.y) / so,pos[tab.z .. +tab.w) in
// the reference's emission order; counters[0..1] must be zeroed.
int rv_scan_multi_launch(Workspace &ws, const sa_t *SA, const lcp_t *LCP, int64_t m, const uint8_t *BWT, const sa_t *nsep, int nsamples,
                         int minl, int minn, RvMultiRec *rec, uint16_t *so, sa_t *pos, u32 rec_cap, u32 mem_cap, u32 *counters, uint4 *tiletab,
                         const int64_t *sub_start, const int *sub_want, int nsubs);   // sub_want != NULL: keep only matches with n == sub_want[sub of ub]

// The reference's default picker in place of the longest full match (k_pick_multi_chain, rv_pick_multi_chain.hip; rv_many's handle under the multi-sample
// chain route): for every sub-index s, from the records an UNFILTERED k_scan_multi left in rec / tiletab, pick_l[s] = the length of the TRIMMED match
// schemes.graphmumpicker splits on (left as it is where nothing is picked: the caller zeroes it), pick_n[s] = its members, pick_pos[s * W ..] = their
// positions in member (rank) order.  nodes: (begin, end) per sample and sub-index (2 W per sub-index, as k_decide_multi reads them).  A sub-index the
// kernel cannot decide sets bits in the flag word of its JOB and gets no pick: 1 the reference's own trim_overlap raises, 2 broken chain or a match
// outside the intervals, 8 twin offsets, 32 more than `cap` candidates, 64 an interval of 2^17 positions or more.  job_begin[q * njobs + j]: where
// sequence q of job j begins in the text, every row ascending (a job without a q-th sequence: the begin of the next one that has it).  cap: at most
// RV_PICK_MCHAIN_CAP_MAX (RV_PICK_WCHAIN_CAP_MAX with more than RV_PICK_MCHAIN_KMAX samples; RV_PICK_MCHAIN_CAP lowers either: test hook).
#define RV_PICK_MCHAIN_CAP_MAX 512
#define RV_PICK_MCHAIN_WMAX 512        // (rv_pick_multi_chain.hip derives it: 2^17 ranks x 120 pairs do not keep the scores in 32 bits at RV_LEAF_MCHAIN_WMAX)
#define RV_PICK_MCHAIN_KMAX 16
// ... and of the kernel's 64-sample form (rv_many's RV_MANY_CHAIN_WIDE_LARGE rounds: more than RV_PICK_MCHAIN_KMAX samples): the cap that keeps 64 coordinates a
// candidate in LDS, and the weight bound rv_pick_multi_chain.hip derives for 2^17 ranks x 2016 pairs
#define RV_PICK_WCHAIN_CAP_MAX 256
#define RV_PICK_WCHAIN_WMAX 128
#define RV_PICK_WCHAIN_KMAX 64
struct RvPickMultiChainArgs {
    const sa_t *nodes; int W;
    int32_t wscore, wpen;                                    // 0 .. RV_PICK_MCHAIN_WMAX (W > RV_PICK_MCHAIN_KMAX: RV_PICK_WCHAIN_WMAX)
    int gcmodel;                                             // 0 sumofpairs, 1 star-avg, 2 star-med
    u32 cap;
    u32 *job_flags; const int64_t *job_begin; int njobs;
};
int rv_pick_multi_chain_launch(Workspace &ws, const sa_t *SA, const RvMultiRec *rec, u32 rec_cap, const uint4 *tiletab, int64_t ntile, const int64_t *sub_start,
                               int nsubs, u32 *pick_l, u32 *pick_n, sa_t *pick_pos, const RvPickMultiChainArgs &c);

// getmultimems (reveal.c:292-434), a stack machine per run of LCP values of minl and more (rv_mems.hip); counts beyond the capacities are still counted.
// Any number of samples a record's 16-bit sample field can name
#define RV_MEMS_MAX_SAMPLES 65536
int rv_multimems_launch(Workspace &ws, const sa_t *SA, const lcp_t *LCP, const uint8_t *BWT, int64_t n, const sa_t *nsep, int nsamples, int minl, int minn,
                        u32 maxlcp, u32 *rec_l, int32_t *rec_c, int64_t *rec_first, uint16_t *so, sa_t *pos,
                        unsigned long long rec_cap, unsigned long long mem_cap, unsigned long long *out);

// Built-in picker for more than two samples: per sub-index the longest match present in every one of its samples
// (ties: smallest minimum position).  pick_l[s] = its length (0 = none), pick_pos[s*nsamples ..] = its members in SA order.
// *cand_count > cand_cap afterwards: the candidate list was too small, grow and rerun.
struct RvMultiCand;
int rv_multi_pick_launch(Workspace &ws, const sa_t *SA, const lcp_t *LCP, int64_t m, const uint8_t *BWT, const sa_t *nsep, int nsamples, int minl, int minn,
                         const int64_t *sub_start, const int *sub_want, int nsubs, const int *tile_sub /* sub-index of rank t * RV_TSUB_TILE */,
                         unsigned long long *best, u32 *pick_l, sa_t *pick_pos, RvMultiCand *cand, u32 cand_cap, u32 *cand_count,
                         hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);      // both given: start / stop of the streaming kernel itself
#define RV_MULTI_CAND_BYTES 16
// Full matches of a whole index with k samples (2 <= k <= 16; the anchor cascade's root list, rv_cascade_multi.hip): every LCP interval of exactly k
// ranks with a value of minl or more whose members are of k different samples and left-maximal.  Entry i of region r (nregions a power of two, counters
// region_cnt[r * cnt_stride] zeroed by the caller -- 64 words apart they sit in different L2 channels; entries beyond rcap are counted, not stored)
// lives at r * rcap + i: c_len = the value, c_pos[.. * k + s] = the member of sample s.
int rv_full_list_launch(Workspace &ws, const sa_t *SA, const lcp_t *LCP, const uint8_t *BWT, int64_t n, const sa_t *nsep, int k, u32 minl,
                        u32 *c_len, sa_t *c_pos, u32 rcap, u32 *region_cnt, int nregions, int cnt_stride, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
#define RV_MULTI_REGIONS 64      // the picker's candidate list: regions with a counter each (counter r at word 64 * r, the largest count at word 64 * RV_MULTI_REGIONS)
