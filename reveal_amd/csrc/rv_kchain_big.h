// rv_kchain_big.h -- the chaining programme of rv_kchain.hip for lists above the caps of k_many_kchain: the host preparation both legs share
// (rv_kchain.hip kc_prepare / kc_backtrack) and the device programme in device memory, tile by tile (rv_kchain_big.hip).  DESIGN.md 3j.
#pragma once
#include "rv_kchain.h"
#include <vector>

// One list after the preparation: the kept records (chain.py:236-245), their points relative to each sequence's begin with p2 appended as point m
// (:249-262), the order of the targets (stable by dimension 0) and the kd order (the leaves of utils.kdtree as range_search hands them out).
struct KcPrep {
    int k = 0, m = 0;
    std::vector<int64_t> kept;        // record of point i < m
    std::vector<int64_t> P;           // point i: P[i k .. i k + k)
    std::vector<int64_t> L;           // its length; L[m] = 0
    std::vector<int> order, kd;       // m + 1 points each
    int refuse = 0;                   // RV_KCHAIN_REFUSE_*: why the device programme does not take the list (0: it does)
};

// the preparation.  m == 0: P holds p2 alone and order / kd stay empty (chain() scores nothing).  weights: for the score bound of `refuse`.  -1: error set
int kc_prepare(int k, int64_t nrec, const uint32_t *l, const int32_t *n, const int64_t *off, const int64_t *pos, const int64_t *lens, int64_t maxmums,
               int64_t wpen, int64_t wscore, KcPrep &out);
// the programme on the host: score / back per point (back: a point, or -1 for p1).  -1: error set
int kc_programme_host(const KcPrep &pp, int64_t wpen, int64_t wscore, int gcmodel, std::vector<int64_t> &score, std::vector<int> &back);
// the path from p2's back-pointer, with the checks (a pointer outside the list, a cycle); -> nodes, or -1
int64_t kc_backtrack(const KcPrep &pp, const std::vector<int64_t> &score, const std::vector<int> &back, uint32_t *out_l, int64_t *out_pos, int64_t *out_score,
                     int64_t *end_score);
// -wpen gapcost(p1, p2): the end score of a list without a kept record
int64_t kc_empty_end(const KcPrep &pp, int64_t wpen, int gcmodel);

// Device buffers of the big programme, kept by the caller between calls
struct RvKchainBigBufs {
    DBuf in, state, out, lists;
    void release() { in.release(); state.release(); out.release(); lists.release(); }
};

// The device programme over every list of `lists` at once (each admitted: refuse == 0, m >= 1): score / back per list as kc_programme_host gives them.
// Launches: the tiles of the longest list, added to *launches
int rv_kchain_big_run(Workspace &ws, RvKchainBigBufs &B, const std::vector<const KcPrep *> &lists, int64_t wpen, int64_t wscore, int gcmodel,
                      std::vector<std::vector<int64_t>> &score, std::vector<std::vector<int>> &back, int64_t *launches);
