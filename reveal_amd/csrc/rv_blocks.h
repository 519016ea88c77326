// rv_blocks.h -- diagonal clusters of `reveal transform` (transform.py addctginfo + clustermumsbydiagonal) on the device: rv_blocks.hip
#pragma once
#include "rv_common.h"
#include "rv_scan.h"
#include <vector>

// what the rule reads besides the records
struct RvBlkArgs {
    int o;                        // 0: forward MUMs (diagonals a - b), 1: reverse-complement MUMs (anti-diagonals a + b + l)
    int cluster;                  // 0: one block per MUM in ascending b, nothing dropped
    int64_t maxdist, minclustsize;
};
// the blocks of one call on the host, in the rule's order
struct RvBlkOut {
    std::vector<int64_t> s1, e1, s2, e2, score;
    std::vector<int32_t> refid, ctgid;
    int64_t nmums = 0, nclusters = 0;      // records read, clusters before the minclustsize filter
    void clear() { s1.clear(); e1.clear(); s2.clear(); e2.clear(); score.clear(); refid.clear(); ctgid.clear(); nmums = nclusters = 0; }
};

// Where the records are.  recs != NULL: the dense list the pair scan's compaction leaves (n of them), b still in the coordinates of the scanned
// text: with rc_map set, b := nsep0 + (nT - b - l) (reveal.c:98-100) as the records are read.  recs == NULL: l / a / b on the HOST, b already
// mapped (what getmums returns); they are uploaded.
struct RvBlkIn {
    const RvPairRec *recs = nullptr;
    int rc_map = 0; int64_t nsep0 = 0, nT = 0;
    const uint32_t *l = nullptr; const int64_t *a = nullptr, *b = nullptr;
    int64_t n = 0;
    int64_t max_a = 0, max_b = 0, max_l = 0;      // upper bounds of the three fields (they size the sort key)
};

// The device programme: keys -> the library's stable radix sort -> heads -> two prefix sums -> one thread per cluster -> ordered compaction.
// end[0 .. nseq): the position of the '$' of every sequence in order of addition (host).  Only the counts and the kept blocks are copied back.
// A pair of records overlapping on one diagonal inside one pair of sequences is an error (the reference's assert).
int rv_blocks_device(Workspace &ws, const RvBlkIn &in, const int64_t *end, int64_t nseq, const RvBlkArgs &args, RvBlkOut &out);

// The same rule in host C++ (no device is asked for).
int rv_blocks_rule_host(int64_t n, const uint32_t *l, const int64_t *a, const int64_t *b, const int64_t *end, int64_t nseq, const RvBlkArgs &args, RvBlkOut &out);
